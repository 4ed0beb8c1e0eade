#!/usr/bin/env python3
"""bench.py — headline benchmark: unique samples/s through log-psi eval + E_loc on N2 (20 qubits),
M = 10 000 unique samples per GPU (BASELINE.json configs[1]).

    python bench.py --gpus N --steps K --warmup W          # N > 1: starts its own N ranks (one per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   # or under torchrun

One "step" = one pass of the hot path over one batch of M unique sampled bit-strings that is already resident
in HBM: (log-psi evaluation of the batch ->) hash build -> matrix-free E_loc -> weighted energy accumulators.

Modes
  default        K independent batches per rank (4 distinct key sets, rotated), `--pipeline` of them in flight on as
                 many HIP streams; with N > 1 every rank owns its own batch stream (weak scaling: the 14 400-state N2
                 space cannot supply N x 10 000 unique samples for one table) and the per-step accumulators [K, 4]
                 are summed over the ranks by one RCCL all-reduce at the end of the timed region.  Before the warm-up
                 the step runs 2 000 times one batch at a time: what brings a freshly started GPU to its sustained
                 state.  With `--full` the same process also measures, and reports inside the same JSON line,
                   * `serial`: those 2 000 steps timed (kernel durations with the GPU to themselves);
                   * `config4_row_sharded`: BASELINE config 4 / north_star's split — ONE Li2O table of 50 000 keys,
                     rows sharded over the ranks (below) — so that a 1/2/4/8-GPU sweep of the default command also
                     yields the strong-scaling curve of the sharded table.
  --shard rows   the sharded table as the primary measurement: every rank evaluates log psi for its contiguous row
                 shard, ONE all-gather assembles the (log|psi|, phase) table (M x 8 B), every rank runs
                 `naqs_eloc` for its rows against the whole table, ONE all-reduce per step sums the 4 energy
                 accumulators.  Total work is fixed -> "scaling": "strong".

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the `--steps` steps and reports the headline
(`metric`, `value`, `unit`, `ms_per_step`, `dtype`, ...), nothing else.  `--full` adds what takes work of its own: the
kernel-duration brackets of the timed region and the `roofline` built on them, `serial`, `config4_row_sharded`,
`train_step` and `cpu_baseline`; everything in it is measured by this run except the fields tagged `"replayed": true`
(hardware counters, which only a rocprofv3 --pmc pass can produce: they are read from the committed profiles/ file
named beside them).  `--dump-outputs DIR` writes what the timed path returned in its last step (log psi, E_loc, the
weighted sums) as DIR/<name>.npy; the inputs are seeded, so two builds can be compared output for output.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "naqs-for-quantum-chemistry_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s achievable
PROF_STRIDE = 10
MFMA_BF16_PEAK_TF = 2500.0  # dense bf16 / f16 MFMA peak (MI355X_MICROARCH.md: "Peak BF16/FP16 MFMA ~2.5 PF dense")
MFMA_F32_PEAK_TF = 157.3   # f32-in/f32-acc MFMA dense peak (MI355X_MICROARCH.md: = the f32 vector rate)
N_CU, SIMD_PER_CU, VALU_CYCLES_PER_WAVE_INST, MAX_CLOCK_HZ = 256, 4, 2, 2.4e9   # MI355X_MICROARCH.md (SIMD-32: 2 cycles)
N_KEY_SETS = 4
PMC_TRAFFIC = "profiles/r06_pmc_traffic.json"
PMC_ISSUE = "profiles/r06_pmc_issue.json"


def phase_format(kernel_name=None):
    """Split format of the log-psi kernel: 2 = f16x2 (three f16 MFMA products per f32 product), 1 = bf16x3 (six bf16
    products), 0 = exact-f32 MFMA.  Read from the name of the kernel that RAN (`naqs_net_last_kernel`: the library falls back
    to the f32 kernel when a split format's planes do not fit the LDS); NAQS_PHASE_MODE (default 2) only before any launch."""
    if kernel_name:
        if "f16x2" in kernel_name:
            return 2
        if "bf16x3" in kernel_name:
            return 1
        if "f32 MFMA" in kernel_name:
            return 0
    return int(os.environ.get("NAQS_PHASE_MODE", "2"))


# ------------------------------------------------------------------------------------------------------------------
# workload
# ------------------------------------------------------------------------------------------------------------------
def physical_keys(n_qubits, n_alpha, n_beta):
    from itertools import combinations
    al = [sum(1 << b for b in c) for c in combinations(range(0, n_qubits, 2), n_alpha)]
    be = [sum(1 << b for b in c) for c in combinations(range(1, n_qubits, 2), n_beta)]
    return np.sort(np.array([a | b for a in al for b in be], np.uint64))


def make_batch(ham, M, seed):
    """keys = sort(RandomState(1234).choice(all physical keys, M)); synthetic
    psi: log|psi| ~ N(-ln(M)/2, 2), phase ~ U[0, 2pi)."""
    n_orb = ham.n_qubits // 2
    from math import comb
    if comb(n_orb, ham.n_alpha) * comb(n_orb, ham.n_beta) <= 2_000_000:
        space = physical_keys(ham.n_qubits, ham.n_alpha, ham.n_beta)
        keys = np.sort(np.random.RandomState(1234 + seed).choice(space, M, replace=False))
    else:
        # config C4 (Li2O: 41 409 225 states): M distinct keys, alpha part = random n_alpha-subset of the even
        # bits, beta part = random n_beta-subset of the odd bits (vectorised: random scores, the smallest n win)
        rs0 = np.random.RandomState(1234 + seed)
        keys = np.zeros(0, np.uint64)
        while len(keys) < M:
            n = int((M - len(keys)) * 1.1) + 16
            a = np.argsort(rs0.random_sample((n, n_orb)), axis=1)[:, :ham.n_alpha]
            b = np.argsort(rs0.random_sample((n, n_orb)), axis=1)[:, :ham.n_beta]
            k = (np.uint64(1) << (2 * a).astype(np.uint64)).sum(1) | (np.uint64(1) << (2 * b + 1).astype(np.uint64)).sum(1)
            keys = np.unique(np.concatenate([keys, k.astype(np.uint64)]))
        keys = np.sort(rs0.permutation(keys)[:M])
    rs = np.random.RandomState(4321 + seed)
    log_psi = np.stack([rs.normal(-0.5 * np.log(M), 2.0, M), rs.uniform(0, 2 * np.pi, M)], -1).astype(np.float32)
    counts = rs.poisson(5, M) + 1
    return keys, log_psi, counts


def algorithmic_bytes(M, K, Kxy):
    """per sample 8 B key + 16 B psi in, 16 B E_loc out, and per candidate connection
    one 8 B key probe + one 16 B psi fetch; the packed term table once per launch."""
    return M * (40 + 24 * Kxy) + 16 * K + 12 * Kxy


def logpsi_flops(n_qubits, M, amp_in_kernel=True):
    """phase MLP 2*(K*N) flops per layer and sample (18->512->512->4 for N2) + the amplitude blocks
    (pair n: 2n -> 64 -> 5) evaluated in the same launch."""
    dims = [max(1, 2 * (n_qubits // 2 - 1)), 512, 512, 4]
    f = 2.0 * M * sum(a * b for a, b in zip(dims, dims[1:]))
    if amp_in_kernel:
        f += 2.0 * M * sum(max(1, 2 * n) * 64 + 64 * 5 for n in range(n_qubits // 2))
    return f


def logpsi_executed_flops(n_qubits, M, fmt=None, out_layer_on_valu=False):
    """16-bit flops the matrix cores execute for the same launch.  f16x2 (fmt 2): every f32 product is three f16 products
    (two where one operand is exact in f16: the +-1 / 0 inputs of the phase MLP's first layer and of the amplitude blocks'
    first layer); bf16x3 (fmt 1): six (three) bf16 products in the phase MLP — the amplitude blocks are f16x2 in both."""
    fmt = phase_format() if fmt is None else fmt
    full, exact = (3, 2) if fmt == 2 else (6, 3)
    P = n_qubits // 2
    dims = [max(1, 2 * (P - 1)), 512, 512, 4]
    # phase_kernel_ws forms the 512 -> 4 output layer from the accumulators with f32 FMAs: not matrix-core work
    f = 2.0 * M * (exact * dims[0] * dims[1] + full * dims[1] * dims[2] + (0 if out_layer_on_valu else full * dims[2] * dims[3]))
    f += 2.0 * M * sum(2 * max(1, 2 * n) * 64 + 3 * 64 * 5 for n in range(P))
    return f


def published_ansatz(ham_p):
    # experiments/bash/naqs/batch_train.sh:14: amplitude blocks 1x64, one phase block 2x512
    return dict(qubit_ordering=-1, amp_hidden_size=[64], phase_hidden_size=[512, 512], use_amp_spin_sym=True,
                use_phase_spin_sym=False, aggregate_phase=False, n_alpha_electrons=ham_p.n_alpha,
                n_beta_electrons=ham_p.n_beta)


def shard_rows(M, rank, world):
    """Equal padded shards (an all-gather needs equal contributions): rank r evaluates log psi for rows
    [r*S, (r+1)*S) of the table padded to S*world rows and owns E_loc rows [r*S, min(M, (r+1)*S))."""
    S = -(-M // world)
    b = min(M, rank * S)
    return S, b, min(M, b + S)


# ------------------------------------------------------------------------------------------------------------------
# CPU leg
# ------------------------------------------------------------------------------------------------------------------
def cpu_baseline(ham_p, keys, log_psi, wf_args, budget_s=16.0):
    """CPU leg, same two stages as the GPU step, on the host cores of this box, bounded sample:
      * E_loc: the oracle's staged restatement of the reference algorithm (update_H + get_H + SpMV
        with a cold Hamiltonian cache — equal work to the matrix-free GPU path), OpenMP;
      * log-psi eval: the same torch modules the reference would run on CPU (its nade.py is PyTorch),
        float32, torch intra-op threads.
    Timed twice: on all host threads and pinned to 8 threads (the box-independent figure BASELINE.md asks for;
    the build container's 8-core numbers for the reference itself are in BASELINE.md / tests/golden/kat.json)."""
    import torch
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    from oracle import oracle
    psi = np.exp(log_psi[:, 0].astype(np.float64)) * np.exp(1j * log_psi[:, 1].astype(np.float64))
    # the whole batch the GPU leg runs, unless the reference algorithm's M*Kyz parity bytes + M*Kxy (double + int32) matrix
    # entries would pass ~2 GB (Li2O tables): then the first rows that fit (said in `sample`)
    n_xy, n_yz = len(np.unique(ham_p.xy)), len(np.unique(ham_p.yz))
    Ms = min(len(keys), max(1000, int(2e9 // (n_yz + 12 * n_xy))))
    k, p = keys[:Ms], psi[:Ms]
    all_threads = int(oracle.max_threads())
    torch_all = torch.get_num_threads()
    args = (ham_p.n_qubits, ham_p.n_alpha, ham_p.n_beta, ham_p.xy, ham_p.yz, ham_p.coeff, k, p)
    hil = Hilbert.get(ham_p.n_qubits, ham_p.n_alpha, ham_p.n_beta, encoding=Encoding.SIGNED)
    wf = NAQSComplex_NADE_orbitals(hil, device="cpu", **wf_args)
    states = hil.idx2state(torch.from_numpy(k.astype(np.int64)))

    def timed(fn, budget):
        fn()
        reps, t0 = 0, time.perf_counter()
        while True:
            fn()
            reps += 1
            dt = time.perf_counter() - t0
            if dt > budget or reps >= 100:
                return dt / reps, reps

    def leg(threads, torch_threads, budget):
        oracle.set_threads(threads)
        torch.set_num_threads(torch_threads)
        t_e, r_e = timed(lambda: oracle.eloc_staged(*args), budget / 2)
        with torch.no_grad():
            t_l, r_l = timed(lambda: wf.log_psi(states), budget / 2)
        return {"value": Ms / (t_e + t_l), "cores": int(threads), "eloc_ms": t_e * 1e3, "logpsi_ms": t_l * 1e3,
                "eloc_reps": r_e, "logpsi_reps": r_l, "torch_threads": int(torch_threads),
                "eloc_only_samples_per_s": Ms / t_e, "logpsi_only_samples_per_s": Ms / t_l}

    try:
        full = leg(all_threads, torch_all, budget_s * 0.6)
        eight = leg(min(8, all_threads), min(8, torch_all), budget_s * 0.4)
    finally:
        oracle.set_threads(all_threads)
        torch.set_num_threads(torch_all)
    best = full if full["value"] >= eight["value"] else eight       # the harder baseline is the one reported as `value`
    keep = ("value", "cores", "eloc_ms", "logpsi_ms", "torch_threads")
    return {"value": best["value"], "unit": "unique samples/s", "cores": best["cores"], "kind": "port",
            "sample": f"{'the whole batch of' if Ms == len(keys) else 'first'} {Ms} samples{'' if Ms == len(keys) else ' of the batch'}: {best['eloc_reps']} x E_loc (oracle staged restatement of "
                      f"update_H+get_H+SpMV, cold cache, {best['cores']} OpenMP threads, {best['eloc_ms']:.1f} ms each) + "
                      f"{best['logpsi_reps']} x log-psi eval (torch CPU float32, {best['torch_threads']} threads, "
                      f"{best['logpsi_ms']:.1f} ms each); timed on all host threads and on 8 — the faster leg is `value`",
            "eloc_only_samples_per_s": best["eloc_only_samples_per_s"],
            "logpsi_only_samples_per_s": best["logpsi_only_samples_per_s"],
            "all_threads": {k_: full[k_] for k_ in keep}, "eight_threads": {k_: eight[k_] for k_ in keep}}


# ------------------------------------------------------------------------------------------------------------------
# the training step (what real runs execute: PartialSamplingOptimizer.run, src/optimizer/energy.py:902-1056)
# ------------------------------------------------------------------------------------------------------------------
def train_step_probe(dev, molecule, steps=300, warmup=40, n_samples=1000000):
    """ms per VMC training step of the published ansatz on `molecule` through the optimiser's own loop (sampler -> forward +
    E_loc -> backward -> Adam -> re-pack; `naqs_vmc_run` / `naqs_vmc_step`), after `warmup` steps from a random
    initialisation (seed 1): the regime of a run's first few hundred steps, tables of 10^3 .. 10^4 unique samples.
    Beside it: the sampler's share (HIP events around its launches on every 10th step: first sampler launch .. the launch that
    writes the weights) and the kernel launches per step (the library's own counter over the timed region)."""
    import contextlib
    import io
    import torch
    from naqs_amd import _lib
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.nade import NadeMasking
    from naqs_amd.optimizer import LogKey, PartialSamplingOptimizer
    from naqs_amd.system import load_molecule, set_global_seed
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    lib = _lib.load_library()
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        set_global_seed(1)
        mol, qh = load_molecule(os.path.join(ROOT, "tests", "golden", f"ham_{molecule}.npz"))
        na, nb = mol.get_n_alpha_electrons(), mol.get_n_beta_electrons()
        hil = Hilbert.get(N=mol.n_qubits, N_alpha=na, N_beta=nb, encoding=Encoding.SIGNED)
        wf = NAQSComplex_NADE_orbitals(hil, qubit_ordering=-1, masking=NadeMasking.PARTIAL, use_amp_spin_sym=True,
                                       use_phase_spin_sym=False, n_alpha_electrons=na, n_beta_electrons=nb, device=dev,
                                       amp_hidden_size=[64], phase_hidden_size=[512, 512], aggregate_phase=False)
        opt = PartialSamplingOptimizer(n_samples=n_samples, n_samples_max=1e12, n_unq_samples_min=1000, n_unq_samples_max=1e5,
                                       wavefunction=wf, qubit_hamiltonian=qh, pre_compute_H=False, n_electrons=mol.n_electrons,
                                       n_alpha_electrons=na, n_beta_electrons=nb, optimizer=torch.optim.Adam,
                                       optimizer_args=[{'lr': 1e-3, 'betas': (0.9, 0.99), 'eps': 1e-15}, {'lr': 1e-2}],
                                       save_loc=os.path.join(os.environ.get("TMPDIR", "/tmp"), f"naqs_bench_train_{molecule}_{os.getpid()}"),
                                       seed=1, grad_clip_factor=None, log_exact_energy=False, pauli_hamiltonian_dtype=np.float64,
                                       normalise_psi=True)
        opt.run(warmup, output_freq=10 ** 9)
        fused = wf.fused(need_phase=True)
        path = ("naqs_vmc_run (the loop in the library)" if opt._can_onecall() and opt._can_run_in_library()
                else "naqs_vmc_step per step" if opt._can_onecall() else "library calls per stage")
        _lib.check(lib.naqs_net_prof_select(fused._h, 1), "naqs_net_prof_select")
        fused.prof_enable(steps // PROF_STRIDE + 2, PROF_STRIDE)
        torch.cuda.synchronize()
        l0, t0 = lib.naqs_launch_count(), time.perf_counter()
        opt.run(steps, output_freq=10 ** 9)
        torch.cuda.synchronize()
        dt, l1 = time.perf_counter() - t0, lib.naqs_launch_count()
        s_ms, s_n = fused.prof_read()
        fused.prof_enable(0)
        _lib.check(lib.naqs_net_prof_select(fused._h, 0), "naqs_net_prof_select")
        # the training forward is queued behind the sampler before the host knows M (naqs_net_spec_counts): launched / stood
        spec = (ctypes.c_int64 * 2)()
        _lib.check(lib.naqs_net_spec_counts(fused._h, spec), "naqs_net_spec_counts")
    m = [x[1] for x in opt.log[LogKey.N_UNIQUE_SAMP][-steps:]]
    return {"ms_per_step": dt / steps * 1e3, "steps": steps, "warmup": warmup, "sampler_us": s_ms / max(s_n, 1) * 1e3,
            "launches_per_step": (l1 - l0) / steps, "unique_samples_mean": float(np.mean(m)), "unique_samples_last": int(m[-1]),
            "n_samples": int(opt.n_samples), "E_loc_last": float(opt.log[LogKey.E_LOC][-1][1]), "path": path,
            "forward_ahead_of_M": {"launched": int(spec[0]), "stood": int(spec[1]), "over": "warm-up + timed steps"},
            "sampler_us_note": "the sampler's own launches; its one-workgroup finish job rides in the forward launch"}


# ------------------------------------------------------------------------------------------------------------------
# self-launch: `python bench.py --gpus N` with N > 1 and no launcher in the environment
# ------------------------------------------------------------------------------------------------------------------
def launch_ranks(n, argv):
    """Start one child process per GPU (rank r -> LOCAL_RANK r) and wait for them.  The parent never touches the GPU
    (no HIP call before or after the children start — a process that has initialised the GPU must not exec or fork
    GPU work).  Rank 0's stdout is passed through, so its JSON line stays the last line of ours; the other ranks'
    output goes to stderr."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    base = dict(os.environ, WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), NAQS_BENCH_CHILD="1")
    procs = []
    for r in range(n):
        env = dict(base, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=None if r == 0 else sys.stderr))
    # poll all ranks together: the first failing one ends the launch (the others would sit in a collective until the
    # deadline); fresh children only, never a re-exec
    deadline = time.time() + float(os.environ.get("NAQS_BENCH_LAUNCH_TIMEOUT", "3600"))
    codes = [None] * n
    while any(c is None for c in codes):
        for i, pr in enumerate(procs):
            if codes[i] is None:
                codes[i] = pr.poll()
        failed = [c for c in codes if c not in (None, 0)]
        if failed or time.time() > deadline:
            for i, pr in enumerate(procs):
                if codes[i] is None:
                    pr.kill()
                    pr.wait()
                    codes[i] = 124 if not failed else -9
            break
        time.sleep(0.05)
    bad = [c for c in codes if c != 0]
    if bad:
        print(f"bench.py: rank exit codes {codes}", file=sys.stderr)
        first = next(c for c in codes if c not in (0, -9)) if any(c not in (0, -9) for c in codes) else bad[0]
        return first
    return 0


def dry_run(args, world, rank):
    """NAQS_BENCH_DRY_RUN=1 (tests/test_bench.py, no GPU): the ranks the launcher started form a gloo group and push
    the sharded step's collectives through it with the real shapes — padded row shards all-gathered into the
    (log|psi|, phase) table, 4 accumulators all-reduced per step — on closed-form stand-in values, so that shard
    bounds, gather order and the reduction can be checked exactly.  Nothing is measured: "value" is null."""
    import torch
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    M = args.samples
    S, b, e = shard_rows(M, rank, world)
    rows = torch.arange(rank * S, (rank + 1) * S, dtype=torch.float64)
    mine = torch.stack([rows * 0.5, -rows], -1)                       # stand-in (log|psi|, phase) of my padded shard
    table = torch.empty((S * world, 2), dtype=torch.float64)
    if world > 1:
        dist.all_gather_into_tensor(table, mine)
    else:
        table.copy_(mine)
    want = torch.arange(S * world, dtype=torch.float64)
    ok_table = bool(torch.equal(table[:, 0], want * 0.5) and torch.equal(table[:, 1], -want))
    acc = torch.zeros((args.steps, 4), dtype=torch.float64)
    r = torch.arange(b, e, dtype=torch.float64)
    for i in range(args.steps):
        acc[i] = torch.stack([r.sum() * (i + 1), (r * r).sum(), torch.tensor(float(e - b)), torch.tensor(1.0)])
        if world > 1:
            dist.all_reduce(acc[i])
    full = torch.arange(M, dtype=torch.float64)
    ok_acc = bool(acc[-1, 0] == full.sum() * args.steps and acc[-1, 1] == (full * full).sum()
                  and acc[-1, 2] == M and acc[-1, 3] == world)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": "dry run (launcher + collectives wiring; nothing measured)", "value": None,
                          "dry_run": True, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ranks": world, "backend": "gloo", "shard_rows": [S, b, e], "table_ok": ok_table,
                          "accumulators_ok": ok_acc, "shard": args.shard}), flush=True)
    return 0 if (ok_table and ok_acc) else 1


# ------------------------------------------------------------------------------------------------------------------
# the row-sharded table (config 4 / north_star's split)
# ------------------------------------------------------------------------------------------------------------------
def run_row_sharded(dev, world, rank, use_dist, molecule, M, steps, warmup, depth=2, streams=None, emulate=False, prof=True,
                    want_outputs=False):
    """-> dict with ms_per_step, samples/s and the kernel durations of one sharded table of M keys.  `depth` evaluations
    of the table are in flight (one HIP stream and one handle pair each, as in the default mode): the E_loc kernel and the
    collectives of one overlap the log-psi kernel of the next.
    emulate (--emulate-world, single process): this process plays rank `rank` of `world` WITHOUT the others — it evaluates
    log psi for its own padded row shard and E_loc for its own rows against the WHOLE table, which is evaluated once up
    front outside the timed region and stands in for what the all-gather would deliver; no collective is issued.
    prof=False: no kernel-duration brackets in the timed region (the kernel fields read 0).  want_outputs: the dict also
    holds `_outputs`, what the last timed step returned on this rank (the table's log psi, E_loc of its rows, the sums)."""
    import torch
    import torch.distributed as dist
    from naqs_amd import hamiltonian, packing
    from naqs_amd.fused import FusedLogPsi
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    ham_p = packing.load_packed(os.path.join(ROOT, "tests", "golden", f"ham_{molecule}.npz"))
    ham = hamiltonian.DevicePauliHamiltonian(ham_p, device=dev)
    keys_np, log_psi_np, counts_np = make_batch(ham_p, M, seed=0)           # ONE table, the same on every rank
    keys = hamiltonian.keys_to_device(keys_np, dev)
    torch.manual_seed(1234)                                                   # replicated network
    hil = Hilbert.get(ham_p.n_qubits, ham_p.n_alpha, ham_p.n_beta, encoding=Encoding.SIGNED)
    wf_args = published_ansatz(ham_p)
    wf = NAQSComplex_NADE_orbitals(hil, device=dev, **wf_args)
    depth = max(1, depth)
    hams = [ham] + [hamiltonian.DevicePauliHamiltonian(ham_p, device=dev) for _ in range(depth - 1)]
    nets = [FusedLogPsi(wf) for _ in range(depth)]
    # (the caller's streams when it has some: the runtime multiplexes HIP streams onto a few hardware queues — 4 by
    # default — and two streams that land on one queue run one after the other; with the default mode's two streams still
    # alive, two fresh ones for this table shared a queue and nothing overlapped)
    if streams is None or len(streams) < depth:
        streams = [torch.cuda.Stream(device=dev) for _ in range(depth)] if depth > 1 else [torch.cuda.current_stream(dev)]
    S, b, e = shard_rows(M, rank, world)
    pad = S * world - M
    keys_pad = torch.cat([keys, keys[:pad]]) if pad else keys
    my_keys = keys_pad[rank * S:(rank + 1) * S].contiguous()
    lp_mine = [torch.empty((S, 2), dtype=torch.float32, device=dev) for _ in range(depth)]
    table = [torch.empty((S * world, 2), dtype=torch.float32, device=dev) for _ in range(depth)]
    weights = torch.as_tensor(counts_np / counts_np.sum(), dtype=torch.float64, device=dev)
    w_mine = weights[b:e].contiguous()
    eloc = [torch.empty((max(e - b, 0), 2), dtype=torch.float64, device=dev) for _ in range(depth)]
    acc = torch.zeros((warmup + steps, 4), dtype=torch.float64, device=dev)
    for h_ in hams:
        h_.reserve(M)
    full_table = nets[0].log_psi(keys_pad).clone() if emulate and world > 1 else None
    torch.cuda.synchronize()
    pending, to_reduce = [], []

    def step(i):
        d = i % depth
        with torch.cuda.stream(streams[d]):
            nets[d].log_psi(my_keys, out=lp_mine[d])                          # my rows of the table
            if use_dist:
                dist.all_gather_into_tensor(table[d], lp_mine[d])             # the exchange step: M x 8 B in all
                lp_table = table[d]
            else:
                lp_table = lp_mine[d] if full_table is None else full_table
            hams[d].local_energy(keys, lp_table[:M], kind="log_psi", row_begin=b, n_rows=e - b, weights=w_mine, out=eloc[d],
                                 sums_out=acc[i])
        # the all-reduce of a step is issued one step late: torch runs a communicator's collectives in issue order on one
        # internal stream, and a reduce that waits for this step's E_loc would hold back the NEXT step's all-gather there
        # (measured at RCCL world 1: no overlap at all, 0.54 ms/step at any depth)
        if use_dist:
            to_reduce.append((i, d))
            while len(to_reduce) > depth - 1:
                reduce_step(*to_reduce.pop(0))

    def reduce_step(i, d):
        with torch.cuda.stream(streams[d]):
            pending.append(dist.all_reduce(acc[i], async_op=True))            # 32 B

    def fence(barrier=True):
        while to_reduce:
            reduce_step(*to_reduce.pop(0))
        for w_ in pending:
            w_.wait()
        pending.clear()
        torch.cuda.synchronize()
        if use_dist and barrier:
            dist.barrier()
            torch.cuda.synchronize()

    for i in range(warmup):
        step(i)
    fence()
    stride = max(1, min(PROF_STRIDE, (steps // depth) // 4))
    if prof:
        for h_, n_ in zip(hams, nets):
            h_.prof_enable(steps // stride + 1, stride)
            n_.prof_enable(steps // stride + 1, stride)
    t0 = time.perf_counter()
    for i in range(steps):
        step(warmup + i)
    fence(barrier=False)          # the last step's all-reduce is the closing barrier (every rank must have entered it)
    dt = time.perf_counter() - t0
    if use_dist:
        dist.barrier()
    e_ms = e_n = p_ms = p_n = 0
    if prof:
        for h_, n_ in zip(hams, nets):
            a_, b_ = h_.prof_read(); e_ms += a_; e_n += b_; h_.prof_enable(0)
            a_, b_ = n_.prof_read(); p_ms += a_; p_n += b_; n_.prof_enable(0)
    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    if use_dist and world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    s = acc[warmup + steps - 1].cpu().numpy()
    t_eloc, t_lp = e_ms / max(e_n, 1) * 1e-3, p_ms / max(p_n, 1) * 1e-3
    res = {"workload": f"{molecule} STO-3G ({ham.n_qubits} qubits, K={ham.K}, Kxy={ham.Kxy}): ONE table of {M} unique "
                       f"samples, rows sharded over {world} rank(s)",
           "value": M * steps / dt, "unit": "unique samples/s", "ms_per_step": dt / steps * 1e3, "steps": steps,
           "warmup": warmup, "scaling": "strong", "rows_per_rank": int(e - b), "logpsi_rows_per_rank": int(S),
           "pipeline": f"{depth} evaluation(s) of the table in flight on {depth} HIP stream(s)",
           "collectives_per_step": (f"1 all-gather of the (log|psi|, phase) table ({M * 8} B in all) + 1 all-reduce of 4 "
                                    f"accumulators (32 B), {'RCCL' if dist.get_backend() == 'nccl' else dist.get_backend()}, "
                                    f"{dist.get_world_size()} rank(s)") if use_dist else "none (single process)",
           "energy": float(s[0] / s[3]),
           "eloc_kernel_us": t_eloc * 1e6, "logpsi_kernel_us": t_lp * 1e6,
           "eloc_kernel_name": hams[0].last_kernel(), "logpsi_kernel_name": nets[0].last_kernel()}
    b_alg = algorithmic_bytes(e - b, ham.K, ham.Kxy) if e > b else 0
    res["eloc_algorithmic_GBps"] = b_alg / t_eloc / 1e9 if t_eloc > 0 else 0.0
    issue = issue_roofline(f"{molecule}_{M}", t_eloc) if world == 1 and prof else None
    if issue:
        res["eloc_issue"] = issue
    if want_outputs:
        d = (warmup + steps - 1) % depth
        lp_table = table[d] if use_dist else (lp_mine[d] if full_table is None else full_table)
        res["_outputs"] = {"log_psi": lp_table[:M].cpu().numpy(), "e_loc": eloc[d].cpu().numpy(), "sums": s}
    for h_ in hams:
        h_.close()
    for n_ in nets:
        n_.close()
    return res, (ham_p, keys_np, log_psi_np, wf_args)


# ------------------------------------------------------------------------------------------------------------------
# committed hardware-counter files (replayed: only a rocprofv3 --pmc pass can produce them)
# ------------------------------------------------------------------------------------------------------------------
def _load_json(rel):
    try:
        with open(os.path.join(ROOT, rel)) as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def library_source_hash():
    from naqs_amd import _lib
    return _lib.load_library().naqs_source_hash().decode()


def counters_match_library(pmc):
    """A committed counter file is replayed only when it was collected on the kernels this run executes: tools/collect_pmc.py
    stamps it with naqs_source_hash() (SHA-256 prefix of csrc/*.hip, *.hpp) of the library the passes ran."""
    return bool(pmc) and pmc.get("_source_hash") == library_source_hash()


def issue_roofline(workload_key, t_kernel_s):
    """VALU issue utilisation of eloc_kernel = wave-level VALU instructions per launch (SQ_INSTS_VALU of the committed
    --pmc pass, tools/collect_pmc.py) x 2 cycles each (a wave64 VALU instruction occupies its SIMD-32 for 2 cycles,
    MI355X_MICROARCH.md) / (256 CUs x 4 SIMDs x kernel cycles).  `frac_in_counter_pass` takes the kernel cycles from
    the same pass (SQ_BUSY_CYCLES / 32 shader engines): the figure the committed file supports on its own; `frac`
    re-prices the same instruction count against THIS run's kernel duration at the clock the counter pass ran at."""
    pmc = _load_json(PMC_ISSUE)
    if not pmc or workload_key not in pmc or "eloc_kernel" not in pmc[workload_key] or t_kernel_s <= 0:
        return None
    if not counters_match_library(pmc):
        return None
    c = pmc[workload_key]["eloc_kernel"]
    clock = c.get("effective_clock_hz") or MAX_CLOCK_HZ
    per_cycle = N_CU * SIMD_PER_CU / VALU_CYCLES_PER_WAVE_INST                 # VALU wave-instructions the chip can issue per cycle
    out = {"bound": "valu-issue", "valu_insts_per_launch": c["SQ_INSTS_VALU"],
           "frac": c["SQ_INSTS_VALU"] / (per_cycle * t_kernel_s * clock), "clock_hz": clock, "replayed": True,
           "source": PMC_ISSUE, "counters_per_launch": {k: v for k, v in c.items() if k.startswith(("SQ_", "GRBM_"))}}
    if c.get("kernel_cycles"):
        out["frac_in_counter_pass"] = c["SQ_INSTS_VALU"] / (per_cycle * c["kernel_cycles"])
        total = sum(c.get(k, 0.0) for k in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_VMEM"))
        # all instruction classes together, per CU and cycle: the kernel sits at ~1 — one instruction per CU-cycle, i.e.
        # one per SIMD issue turn — with 8 waves per SIMD resident: the bound is the number of instructions, not VALU width
        out["insts_per_cu_cycle"] = total / (N_CU * c["kernel_cycles"])
        out["salu_insts_per_cu_cycle"] = c.get("SQ_INSTS_SALU", 0.0) / (N_CU * c["kernel_cycles"])
    return out


def eloc_roofline(kernel_name, t_kernel_s, rows, K, Kxy, workload_key, t_isolated_s):
    """The local-energy kernel is integer / bit work whose bound is instruction issue: `achieved` = VALU
    wave-instructions per second from the committed counter pass re-priced at this run's kernel duration, `peak` = what
    the chip's SIMD-32s can issue (a wave64 VALU instruction holds its SIMD for 2 cycles).  The survey's algorithmic-bytes
    rate is kept beside it without a fraction: candidates that are rejected in registers never become bytes
    (76 % of them on N2, more on Li2O), so it is not a DRAM rate and can exceed the HBM peak."""
    b_alg = algorithmic_bytes(rows, K, Kxy)
    roof = {"bound": "valu-issue", "achieved": None, "peak": None, "unit": "G VALU wave-instructions/s", "frac": None,
            "traffic": None, "kernel": kernel_name, "kernel_us": t_kernel_s * 1e6,
            "algorithmic_bytes_rate": {"GBps": b_alg / t_kernel_s / 1e9 if t_kernel_s > 0 else 0.0, "bytes_per_launch": b_alg,
                                       "note": "SURVEY 8d bytes / kernel time: an algorithmic rate, not DRAM traffic"}}
    t_use = t_isolated_s if t_isolated_s else t_kernel_s
    issue = issue_roofline(workload_key, t_use) if workload_key else None
    if issue:
        per_cycle = N_CU * SIMD_PER_CU / VALU_CYCLES_PER_WAVE_INST
        roof["achieved"] = issue["valu_insts_per_launch"] / t_use / 1e9
        roof["peak"] = per_cycle * issue["clock_hz"] / 1e9
        roof["frac"] = issue["frac"]
        issue["kernel_us_used"] = t_use * 1e6
        roof["issue"] = issue
    else:
        roof["note"] = ("no committed counter pass for this workload on this library build (source hash "
                        f"{library_source_hash()}): achieved / frac need tools/collect_pmc.py")
    if t_isolated_s:
        roof["isolated"] = {"kernel_us": t_isolated_s * 1e6, "algorithmic_GBps": b_alg / t_isolated_s / 1e9}
    return roof


def logpsi_roofline(kernel_name, t_s, n_qubits, rows, amp_in_kernel, t_isolated_s):
    """`frac` is what the silicon does: executed 16-bit flops (three f16 MFMA products per f32 product in the f16x2 split,
    six bf16 ones in bf16x3) against the dense bf16/f16 MFMA peak — it counts the split's 3x (6x) as useful work.
    `algorithmic_frac` is the same clock without that credit: the network's own f32 flops against the same
    16-bit peak.  The third view — those flops against the f32-MFMA peak, the rate an exact-f32 kernel could reach at most —
    is kept under `f32_equivalent`; it may exceed 1, which only says the kernel is not on the f32 pipe."""
    fmt = phase_format(kernel_name)
    flops = logpsi_flops(n_qubits, rows, amp_in_kernel)
    tf = flops / t_s / 1e12 if t_s > 0 else 0.0
    if fmt == 0:
        return {"bound": "mfma", "achieved": tf, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s", "frac": tf / MFMA_F32_PEAK_TF,
                "algorithmic_frac": tf / MFMA_F32_PEAK_TF, "traffic": None, "kernel": kernel_name, "kernel_us": t_s * 1e6, "algorithmic_flops_per_launch": flops}
    exec_flops = logpsi_executed_flops(n_qubits, rows, fmt, "phase_kernel_ws" in (kernel_name or "")) if amp_in_kernel else flops
    etf = exec_flops / t_s / 1e12 if t_s > 0 else 0.0
    roof = {"bound": "mfma", "achieved": etf, "peak": MFMA_BF16_PEAK_TF, "unit": "TFLOP/s", "frac": etf / MFMA_BF16_PEAK_TF,
            "algorithmic_frac": tf / MFMA_BF16_PEAK_TF, "traffic": None, "dtype_executed": ("f16" if fmt == 2 else "bf16") + " (f32 accumulate)", "kernel": kernel_name,
            "kernel_us": t_s * 1e6, "executed_flops_per_launch": exec_flops, "algorithmic_flops_per_launch": flops,
            "f32_equivalent": {"achieved": tf, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s", "frac": tf / MFMA_F32_PEAK_TF}}
    if t_isolated_s:
        roof["isolated"] = {"kernel_us": t_isolated_s * 1e6, "achieved": exec_flops / t_isolated_s / 1e12,
                            "frac": exec_flops / t_isolated_s / 1e12 / MFMA_BF16_PEAK_TF,
                            "algorithmic_frac": flops / t_isolated_s / 1e12 / MFMA_BF16_PEAK_TF,
                            "f32_equivalent_frac": flops / t_isolated_s / 1e12 / MFMA_F32_PEAK_TF}
    return roof


def dtype_label(kernel_name=None):
    fmt = phase_format(kernel_name)
    net = {2: "f16x2-split MFMA, f32-equivalent", 1: "bf16x3-split MFMA, f32-equivalent", 0: "f32 MFMA"}[fmt if fmt in (0, 1, 2) else 2]
    return f"f32 network ({net}) / f64 E_loc"


def headline_roofline(args, ham, M, lp_name, t_kernel, t_mlp, serial):
    """--full: `roofline` of the default mode from the kernel brackets of the timed region (t_kernel: E_loc, t_mlp: log psi)
    and, where it ran, the serial segment's."""
    amp_in_kernel = "amplitude" in lp_name                            # the kernel's own name says whether the items ran inside it
    eloc_roof = eloc_roofline(ham.last_kernel(), t_kernel, M, ham.K, ham.Kxy, f"{args.molecule}_{M}",
                              serial["eloc_kernel_us"] * 1e-6 if serial and serial["eloc_kernel_us"] > 0 else None)
    mlp_roof = logpsi_roofline(lp_name, t_mlp, ham.n_qubits, M, amp_in_kernel,
                               serial["logpsi_kernel_us"] * 1e-6 if serial and serial["logpsi_kernel_us"] > 0 else None)
    # HBM bytes per launch: hardware counters, from the committed rocprofv3 --pmc passes of this same command
    # (tools/collect_pmc.py; FETCH_SIZE/WRITE_SIZE in separate passes, gfx950 corrections applied there) — replayed only
    # when the file was collected on the library build that is running (source hash)
    pmc = _load_json(PMC_TRAFFIC)
    if counters_match_library(pmc) and args.molecule == "N2" and M == 10000:   # the PMC passes were taken on this workload
        for roof, name in ((eloc_roof, "eloc_kernel"), (mlp_roof, "phase_kernel")):
            if name in pmc:
                roof["traffic"] = pmc[name]["hbm_bytes_per_launch"]
                roof["traffic_source"] = {"replayed": True, "file": PMC_TRAFFIC, "source_hash": pmc["_source_hash"]}
    dominant, other = (mlp_roof, eloc_roof) if t_mlp >= t_kernel else (eloc_roof, mlp_roof)
    roofline = dict(dominant)
    roofline["other_kernels"] = [other]
    return roofline


def dump_outputs(out_dir, arrays):
    """--dump-outputs DIR: what the timed path returned in its last step, as DIR/<name>.npy (float32 / float64 as returned)."""
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


# ------------------------------------------------------------------------------------------------------------------
def worker(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("NAQS_BENCH_DRY_RUN") == "1":
        return dry_run(args, world, rank)

    import torch
    import torch.distributed as dist
    from naqs_amd import hamiltonian, packing

    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # test hook (tests/test_bench.py on the one-GPU box): NAQS_BENCH_ONE_DEVICE=1 puts every rank on device 0 and
    # NAQS_BENCH_BACKEND=gloo carries the collectives (RCCL refuses two ranks per device) — the world > 1 code of both
    # modes then runs on real kernels; the JSON names the backend, such a line is not a multi-GPU measurement
    if os.environ.get("NAQS_BENCH_ONE_DEVICE") == "1":
        local_rank = 0
    backend = os.environ.get("NAQS_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or os.environ.get("NAQS_BENCH_FORCE_DIST") == "1"      # (forced at world 1: exercises the path)
    rank_info = None
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group(backend, rank=rank, world_size=world)
        # what the communicator saw, per rank: (rank, HIP device the rank is bound to, communicator world size) — gathered
        # THROUGH the communicator, so that a recorded line shows that N ranks on N devices took part
        mine = torch.tensor([rank, torch.cuda.current_device(), dist.get_world_size()], dtype=torch.int64,
                            device=dev if backend == "nccl" else "cpu")
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        rank_info = [{"rank": int(t[0]), "device": int(t[1]), "communicator_world_size": int(t[2])} for t in allr]

    if args.emulate_world:
        return emulate_main(args, dev)
    if args.shard == "rows":
        return sharded_main(args, dev, world, rank, use_dist, rank_info)

    ham_p = packing.load_packed(os.path.join(ROOT, "tests", "golden", f"ham_{args.molecule}.npz"))
    ham = hamiltonian.DevicePauliHamiltonian(ham_p, device=dev)
    M = args.samples
    # N_KEY_SETS distinct batches per rank, rotated step by step: consecutive steps never see the same keys, so hash
    # table, psi table and key list are rebuilt from different data every step (nothing is L2-warm from the step before)
    batches = [make_batch(ham_p, M, seed=rank * N_KEY_SETS + j) for j in range(N_KEY_SETS)]
    keys_np, log_psi_np, counts_np = batches[0]                                   # (log_psi_np: CPU-baseline psi only)
    key_sets = [hamiltonian.keys_to_device(b_[0], dev) for b_ in batches]
    weight_sets = [torch.as_tensor(b_[2] / b_[2].sum(), dtype=torch.float64, device=dev) for b_ in batches]
    # ansatz of the published runs (experiments/bash/naqs/batch_train.sh:14): amplitude blocks 1x64,
    # one phase block 2x512, random init (no checkpoints without network) -> log psi of the batch
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    torch.manual_seed(1234 + rank)
    hil = Hilbert.get(ham_p.n_qubits, ham_p.n_alpha, ham_p.n_beta, encoding=Encoding.SIGNED)
    wf_args = published_ansatz(ham_p)
    wf = NAQSComplex_NADE_orbitals(hil, device=dev, **wf_args)
    from naqs_amd.fused import FusedLogPsi
    # Throughput of a STREAM of independent batches: `depth` of them are in flight, each on its own HIP stream with its
    # own handle pair (a handle owns per-call scratch: hash table, psi table), so the E_loc / reduce kernels of one batch
    # run beside the log-psi kernel of the next.  --pipeline 1 = one batch at a time (also measured: `serial`).
    depth = max(1, args.pipeline)
    hams = [ham] + [hamiltonian.DevicePauliHamiltonian(ham_p, device=dev) for _ in range(depth - 1)]
    nets = [FusedLogPsi(wf) for _ in range(depth)]       # libnaqs_hip.so: MFMA log-psi kernel
    streams = [torch.cuda.Stream(device=dev) for _ in range(depth)] if depth > 1 else [torch.cuda.current_stream(dev)]
    log_psis = [torch.empty((M, 2), dtype=torch.float32, device=dev) for _ in range(depth)]
    elocs = [torch.empty((M, 2), dtype=torch.float64, device=dev) for _ in range(depth)]
    for h_ in hams:
        h_.reserve(M)
    torch.cuda.synchronize()
    # energy accumulators: one row of 4 doubles per step, written by the reduce kernel of that step; with N > 1 GPUs the
    # rows of the whole timed region are summed over the ranks by ONE RCCL all-reduce at its end (few, larger
    # collectives: a per-step 32-byte all-reduce is pure xGMI latency and only a training step needs <E> that early)
    n_serial = int(os.environ.get("NAQS_BENCH_NSERIAL", "2000"))
    acc_all = torch.zeros((args.warmup + args.steps + n_serial + 12, 4), dtype=torch.float64, device=dev)
    n_done = [0]

    # The step's ONE library call, naqs_logpsi_eloc(net, ham, M, keys, weights, log psi, E_loc, sums, stream) — phase kernel
    # (amplitude conditionals + phase MLP on the matrix cores; builds the key hash and psi in f64) -> eloc_kernel ->
    # reduce_kernel — through the C ABI with arguments prepared once: what FusedLogPsi.log_psi_and_local_energy does, without
    # the per-call tensor views, stream context and pointer look-ups (~20 us of interpreter per step on a fast host, more than
    # the 31 us step on a slow one: two of seven boxes read 47 us with `--steps 20` and 34 with the default through the wrapper)
    import ctypes
    from naqs_amd import _lib as _naqs_lib
    _call = _naqs_lib.load_library().naqs_logpsi_eloc
    _vp = ctypes.c_void_p
    _acc0 = acc_all.data_ptr()
    _prep = [[(nets[d_]._h, hams[d_]._h, M, _vp(key_sets[k_].data_ptr()), _vp(weight_sets[k_].data_ptr()), _vp(log_psis[d_].data_ptr()),
               _vp(elocs[d_].data_ptr()), _vp(streams[d_].cuda_stream)) for k_ in range(N_KEY_SETS)] for d_ in range(depth)]

    def step(d_override=None):
        i = n_done[0]
        d = (i % depth) if d_override is None else d_override
        nh, hh, m_, kp, wp, lp, ep, sp = _prep[d][i % N_KEY_SETS]
        st = _call(nh, hh, m_, kp, wp, lp, ep, _vp(_acc0 + 32 * i), sp)      # sums -> row i of acc_all (4 doubles)
        if st != 0:
            _naqs_lib.check(st, "naqs_logpsi_eloc")
        n_done[0] += 1

    def fence(first_row=None):
        torch.cuda.synchronize()                 # every stream of this rank
        if use_dist:
            if first_row is not None:
                dist.all_reduce(acc_all[first_row:n_done[0]])
            dist.barrier()
            torch.cuda.synchronize()

    # The same step one batch at a time (single stream, first handle pair), measured in this same run BEFORE the headline
    # region: latency of a batch, and the kernels' durations when each has the GPU to itself.  2000 steps (~0.12 s; env
    # NAQS_BENCH_NSERIAL) whatever --steps says: it is a measurement of its own, and it leaves the GPU in the state a
    # long-running job sees.  A freshly started process needs ~0.1 s of load before the chip reaches its sustained state:
    # with a 200-step segment here `--steps 20 --warmup 5` reads 53-54.5 us/step and the serial step 64.5 us; with 2000,
    # 51.2 and 61.0 — the figures `--steps 400` gives regardless (measured in one gpurun call).
    # (an event pair costs ~4 us of queue time on its stream: at most every 10th launch of a handle is bracketed, and a
    # short region — the driver's `--steps 20` is 10 launches per handle — gets two brackets per handle, not one per step)
    # A plain run keeps the segment as the load that brings the chip to its sustained state, without brackets or report;
    # --full times it and brackets its kernels (`serial`, `roofline.isolated`).
    stride = max(1, min(PROF_STRIDE, (args.steps // depth) // 2))
    import gc
    gc.collect()
    serial = None
    if depth > 1 and not args.no_serial_segment:
        for _ in range(min(args.warmup, 10)):
            step(0)
        fence()
        if args.full:
            hams[0].prof_enable(n_serial // PROF_STRIDE + 1, PROF_STRIDE)
            nets[0].prof_enable(n_serial // PROF_STRIDE + 1, PROF_STRIDE)
        t1 = time.perf_counter()
        for _ in range(n_serial):
            step(0)
        fence()
        dts = time.perf_counter() - t1
        if args.full:
            e_ms, e_n = hams[0].prof_read(); hams[0].prof_enable(0)
            p_ms, p_n = nets[0].prof_read(); nets[0].prof_enable(0)
            serial = {"ms_per_step": dts / n_serial * 1e3, "steps": n_serial, "eloc_kernel_us": e_ms / max(e_n, 1) * 1e3,
                      "logpsi_kernel_us": p_ms / max(p_n, 1) * 1e3, "measured": "this run, before the timed region"}

    # As little host work as possible between the serial segment, the warm-up and the timed region: an idle GPU drops its clocks
    # within a millisecond or so and takes milliseconds of load to come back.  The collector ran before the serial segment and is
    # off until the region closes (a pause inside it would be a third of a 20-step region; a collector RUN between the warm-up
    # and the region — tens of milliseconds — made `--steps 20 --warmup 5` read 39-48 us/step and the default 400 steps 32.6-34,
    # where back-to-back regions of the same process read 32.9 and 30.0: tools/region_probe.py).  What is
    # left between the opening synchronisation and the first timed launch is the creation of the event rings of the kernel-
    # duration brackets (hipEvent pairs on the launch stream around every `stride`-th launch of a handle: a pair costs ~4 us of
    # queue time, recording all of them slows the step by ~15 %): 25-80 us (NAQS_BENCH_VERBOSE=1 prints it).
    gc.disable()                                 # (collected before the serial segment: a collector run here is milliseconds of idle GPU)
    first_warm = n_done[0]
    for _ in range(args.warmup):
        step()
    fence(first_row=first_warm)                  # (also sets the communicator up outside the timed region)
    t_prep = time.perf_counter()
    prof = args.full and os.environ.get("NAQS_BENCH_NOPROF") != "1"     # (diagnostic: --full without the hipEvent brackets)
    if prof:
        for h_, n_ in zip(hams, nets):
            h_.prof_enable(args.steps // stride + 1, stride)
            n_.prof_enable(args.steps // stride + 1, stride)
    if os.environ.get("NAQS_BENCH_VERBOSE") == "1":
        print(f"[bench] host time between the opening synchronisation and the first timed launch: {(time.perf_counter() - t_prep) * 1e6:.0f} us", file=sys.stderr)
    first_timed = n_done[0]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    # closing bracket: this rank's streams drained, then the job's ONE collective — an all-reduce is a barrier (no rank's
    # call completes before every rank has entered it), so a separate dist.barrier() would only add a second collective's
    # latency to a region that may be 1 ms long; MAX over the ranks' clocks below
    torch.cuda.synchronize()
    if use_dist:
        dist.all_reduce(acc_all[first_timed:n_done[0]])
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    gc.enable()
    if use_dist:
        dist.barrier()
    last_row = n_done[0] - 1
    kern_ms = launches = mlp_ms = mlp_launches = 0
    if prof:
        for h_, n_ in zip(hams, nets):
            a, b = h_.prof_read(); kern_ms += a; launches += b
            h_.prof_enable(0)
            a, b = n_.prof_read(); mlp_ms += a; mlp_launches += b
            n_.prof_enable(0)
    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    s = acc_all[last_row].cpu().numpy()
    # what the last timed step's naqs_logpsi_eloc call returned: its pipeline slot's log psi and E_loc, its row of sums
    d_last = last_row % depth
    outputs = {"log_psi": log_psis[d_last].cpu().numpy(), "e_loc": elocs[d_last].cpu().numpy(), "sums": s} \
        if args.dump_outputs and rank == 0 else None
    for h_ in hams[1:]:
        h_.close()
    for n_ in nets[1:]:
        n_.close()

    # BASELINE config 4 in the same run (every rank takes part: it has collectives)
    config4 = None
    if args.full and not args.no_config4 and args.molecule == "N2":
        try:
            config4, _ = run_row_sharded(dev, world, rank, use_dist, "Li2O", 50000, steps=max(50, min(args.steps, 100)),
                                         warmup=max(2, min(args.warmup, 10)), depth=depth, streams=streams)
        except Exception as ex:                                          # the headline must survive a secondary failure
            config4 = {"error": f"{type(ex).__name__}: {ex}"}

    out = None
    if rank == 0:
        lp_name = nets[0].last_kernel()
        out = {
            "metric": f"unique samples/sec through E_loc + log-psi eval ({args.molecule}, {ham.n_qubits} qubits)",
            "value": world * M * args.steps / dt,
            "unit": "unique samples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": dtype_label(lp_name), "data": "synthetic",
            "config": {"workload": f"{args.molecule} STO-3G ({ham.n_qubits} qubits, K={ham.K} Pauli terms, "
                                   f"Kxy={ham.Kxy}), {M} unique samples per GPU, 1xMI355X per rank",
                       "stages": "fused NADE log-psi eval (amp 1x64, phase 2x512; builds the key hash + psi table) + matrix-free E_loc "
                                 "(f64) + weighted energy reduction"
                                 + (" + one RCCL all-reduce of the per-step accumulators [K, 4] at the end of the timed region"
                                    if world > 1 else ""),
                       "pipeline": (f"{depth} independent batches in flight on {depth} HIP streams (one handle pair each)"
                                    if depth > 1 else "one batch at a time"),
                       "batches": f"{N_KEY_SETS} distinct key sets per rank, rotated every step",
                       "input": "unique sampled bit-strings (keys) resident in HBM; random-init network",
                       "ranks": (f"{dist.get_world_size()} {'RCCL' if dist.get_backend() == 'nccl' else dist.get_backend()} rank(s)"
                                 if use_dist else "single process, no process group"),
                       "ranks_detail": rank_info,
                       "energy": float(s[0] / s[3])},
        }
        if args.full:
            out["roofline"] = headline_roofline(args, ham, M, lp_name, kern_ms / max(launches, 1) * 1e-3,
                                                mlp_ms / max(mlp_launches, 1) * 1e-3, serial)
        if serial is not None:
            out["serial"] = serial
        if config4 is not None:
            out["config4_row_sharded"] = config4
        if args.full and not args.no_train_step and world == 1:
            # the real workload's step, so that the driver's line carries it (three molecules, ~1 s each)
            ts = {"what": "one VMC training step (sampler + forward + E_loc + backward + Adam + re-pack) of the published ansatz "
                          "through PartialSamplingOptimizer.run, after 40 steps from a random initialisation"}
            for mol_ in ("N2", "H2O", "Li2O"):
                try:
                    ts[mol_] = train_step_probe(dev, mol_)
                except Exception as ex:                                       # the headline must survive a secondary failure
                    ts[mol_] = {"error": f"{type(ex).__name__}: {ex}"}
            out["train_step"] = ts
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(ham_p, keys_np, log_psi_np, wf_args)
    if outputs is not None:
        dump_outputs(args.dump_outputs, outputs)
    finish(out)
    return 0


def sharded_main(args, dev, world, rank, use_dist, rank_info=None):
    """--shard rows: the sharded table is the measurement (BASELINE config 4 with --molecule Li2O --samples 50000)."""
    import torch.distributed as dist
    res, (ham_p, keys_np, log_psi_np, wf_args) = run_row_sharded(dev, world, rank, use_dist, args.molecule, args.samples,
                                                                 args.steps, args.warmup, depth=max(1, args.pipeline),
                                                                 prof=args.full, want_outputs=bool(args.dump_outputs))
    outputs = res.pop("_outputs", None)
    out = None
    if rank == 0:
        rows, S = res["rows_per_rank"], res["logpsi_rows_per_rank"]
        lp_name = res.pop("logpsi_kernel_name", "phase_kernel_h")
        out = {"metric": f"unique samples/sec through E_loc + log-psi eval ({args.molecule}, {ham_p.n_qubits} qubits), one "
                         f"row-sharded table",
               "value": res["value"], "unit": "unique samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": res["ms_per_step"], "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
               "dtype": dtype_label(lp_name), "data": "synthetic",
               "config": {"workload": res["workload"], "collectives_per_step": res["collectives_per_step"],
                          "ranks": (f"{dist.get_world_size()} {'RCCL' if dist.get_backend() == 'nccl' else dist.get_backend()} rank(s)"
                                    if use_dist else "single process, no process group"),
                          "ranks_detail": rank_info, "rows_per_rank": rows, "energy": res["energy"]}}
        if args.full:
            t_eloc, t_lp = res["eloc_kernel_us"] * 1e-6, res["logpsi_kernel_us"] * 1e-6
            K, Kxy = ham_p.K, len(np.unique(ham_p.xy))
            eloc_roof = eloc_roofline(res.pop("eloc_kernel_name", "eloc_kernel2"), t_eloc, rows, K, Kxy,
                                      f"{args.molecule}_{args.samples}" if world == 1 else None, None)
            mlp_roof = logpsi_roofline(lp_name, t_lp, ham_p.n_qubits, S, "amplitude" in lp_name, None)
            dominant, other = (mlp_roof, eloc_roof) if t_lp >= t_eloc else (eloc_roof, mlp_roof)
            out["roofline"] = dict(dominant)
            out["roofline"]["other_kernels"] = [other]
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(ham_p, keys_np, log_psi_np, wf_args)
        if outputs is not None:
            dump_outputs(args.dump_outputs, outputs)
    finish(out)
    return 0


# What a collective costs on the node cannot be measured here (one GPU).  The scaling models carry two things instead, both
# printed in their JSON: (1) the MEASURED floor of each collective on this box — RCCL at world size 1 through
# torch.distributed, i.e. the software path and the kernel launch with nothing on the wire; (2) a stated per-hop model on top:
# a ring over W ranks takes W - 1 steps for an all-gather and 2 (W - 1) for an all-reduce, each step one xGMI hop of ASSUMED
# latency HOP_US plus its nbytes / W at one link's rate (xGMI is point to point: 7 links x ~153 GB/s per GPU, a ring uses one
# per direction).  Everything stays "unmeasured on hardware" for W > 1.
XGMI_LINK_GBS = 153.0
ASSUMED_HOP_US = 2.0
ASSUMED_FLOOR_US = {"all_gather_table": 25.0, "all_reduce_accumulators": 20.0, "all_reduce_gradient": 35.0}     # when no RCCL group can be formed


def measure_collective_floor(dev, table_bytes, grad_bytes, reps=200):
    """us per collective at world size 1 (RCCL; a group of one is formed here when the process has none): the all-gather of a
    (log|psi|, phase) table of `table_bytes`, the all-reduce of the 64-byte accumulator block and the all-reduce of a flat
    gradient of `grad_bytes` — stream-synchronised means over `reps` calls.  -> (dict, how)"""
    import torch
    import torch.distributed as dist
    made = False
    try:
        if not dist.is_initialized():
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
            made = True
        if dist.get_world_size() != 1:
            return dict(ASSUMED_FLOOR_US), "assumed (the process group has more than one rank: no world-1 measurement taken)"
        out = {}
        cases = {"all_gather_table": ("gather", max(8, table_bytes)), "all_reduce_accumulators": ("reduce", 64),
                 "all_reduce_gradient": ("reduce", max(4, grad_bytes))}
        for name, (kind, nbytes) in cases.items():
            a = torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)
            b = torch.empty_like(a)
            fn = (lambda: dist.all_gather_into_tensor(b, a)) if kind == "gather" else (lambda: dist.all_reduce(a))
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            out[name] = (time.perf_counter() - t0) / reps * 1e6
        return out, f"measured: {dist.get_backend()} ({'RCCL' if dist.get_backend() == 'nccl' else dist.get_backend()}) at world size 1 on this box, mean of {reps} back-to-back calls"
    except Exception as ex:                                              # no RCCL here: fall back to the labelled assumptions
        return dict(ASSUMED_FLOOR_US), f"assumed ({type(ex).__name__}: {ex})"
    finally:
        if made:
            dist.destroy_process_group()


def collective_model_us(kind, world, nbytes, floor_us):
    """floor (measured at world 1) + ring steps x (assumed hop latency + that step's bytes at one xGMI link's rate)"""
    if world <= 1:
        return floor_us
    steps = (world - 1) * (2 if kind == "reduce" else 1)
    return floor_us + steps * (ASSUMED_HOP_US + (nbytes / world) / (XGMI_LINK_GBS * 1e3))


def collective_table(worlds, table_bytes, grad_bytes, floor):
    """per world size: the three collectives of a sharded step under the model above (us)"""
    rows = {}
    for W in worlds:
        rows[str(W)] = {"all_gather_table": collective_model_us("gather", W, table_bytes, floor["all_gather_table"]),
                        "all_reduce_accumulators": collective_model_us("reduce", W, 64, floor["all_reduce_accumulators"]),
                        "all_reduce_gradient": collective_model_us("reduce", W, grad_bytes, floor["all_reduce_gradient"])}
    return rows


def emulate_main(args, dev):
    """--emulate-world: rank 0's share of ONE row-sharded table at every requested world size, on one GPU.  The table's
    strong-scaling ceiling is t(1) / t(W) of these per-rank times (kernels only); with the assumed collective latencies
    added per step it becomes the curve SCALE_rNN.json can be held against.  Everything here is single-GPU evidence:
    "unmeasured on hardware" for W > 1."""
    import torch
    worlds = sorted({int(w) for w in args.emulate_world.split(",")})
    rows = []
    # ONE pair of streams for every world size: the runtime multiplexes HIP streams onto a few hardware queues, and fresh
    # streams per measurement can land on one queue (then nothing overlaps — seen as W = 2 reading its serial time)
    shared = [torch.cuda.Stream(device=dev) for _ in range(max(1, args.pipeline))]
    for depth, label in ((1, "one evaluation at a time"), (max(1, args.pipeline), f"{max(1, args.pipeline)} evaluations in flight")):
        for W in worlds:
            res, _ = run_row_sharded(dev, W, 0, False, args.molecule, args.samples, args.steps, args.warmup, depth=depth, emulate=True,
                                     streams=shared[:depth] if depth > 1 else None)
            rows.append({"world": W, "pipeline": depth, "mode": label, "rank0_ms_per_step": res["ms_per_step"],
                         "rows_per_rank": res["rows_per_rank"], "logpsi_rows_per_rank": res["logpsi_rows_per_rank"],
                         "eloc_kernel_us": res["eloc_kernel_us"], "logpsi_kernel_us": res["logpsi_kernel_us"],
                         "eloc_kernel": res["eloc_kernel_name"], "logpsi_kernel": res["logpsi_kernel_name"]})
    # the evaluation path has two collectives per step: the table's all-gather and the accumulators' all-reduce
    floor, how = measure_collective_floor(dev, args.samples * 8, 4)
    table = collective_table(worlds, args.samples * 8, 4, floor)
    for r in rows:
        base = next(x for x in rows if x["world"] == worlds[0] and x["pipeline"] == r["pipeline"])
        r["kernel_only_speedup"] = base["rank0_ms_per_step"] * (worlds[0] / 1.0) / r["rank0_ms_per_step"] if worlds[0] == 1 else None
        coll = (table[str(r["world"])]["all_gather_table"] + table[str(r["world"])]["all_reduce_accumulators"]) * 1e-3
        # serial step: the collectives' latency adds to every step; pipelined: it overlaps the next evaluation's kernels
        # (bench.py issues the all-reduce one step late for exactly that), so the kernel-only time is the model
        t_model = r["rank0_ms_per_step"] + (coll if (r["world"] > 1 and r["pipeline"] == 1) else 0.0)
        r["model_ms_per_step"] = t_model
        r["model_samples_per_s"] = args.samples / (t_model * 1e-3)
        if worlds[0] == 1:
            r["model_speedup"] = base["rank0_ms_per_step"] / t_model
            r["model_efficiency"] = r["model_speedup"] / r["world"]
    out = {"metric": f"scaling model of one row-sharded table ({args.molecule}, {args.samples} unique samples): rank 0's share per "
                     f"world size, measured on ONE GPU",
           "value": rows[-1]["model_samples_per_s"], "unit": "unique samples/s (model, largest world, pipelined)", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": rows[-1]["model_ms_per_step"], "higher_is_better": True,
           "scaling": "strong", "vs_baseline": None, "dtype": dtype_label(), "data": "synthetic",
           "emulated_worlds": worlds, "unmeasured_on_hardware": True,
           "collective_latency": {"world1_floor_us": floor, "world1_floor_source": how,
                                  "model": f"floor + ring steps x ({ASSUMED_HOP_US} us ASSUMED per xGMI hop + (bytes / W) at {XGMI_LINK_GBS} GB/s per "
                                           "link); steps = W - 1 (all-gather), 2 (W - 1) (all-reduce)",
                                  "per_world_us": {w: {k: v for k, v in t.items() if k != "all_reduce_gradient"} for w, t in table.items()}},
           "config": {"workload": f"{args.molecule} STO-3G, ONE table of {args.samples} unique samples; rank 0 of W evaluates log psi for "
                                  f"ceil(M/W) rows and E_loc for its rows against the whole table (stand-in for the all-gather: the "
                                  f"table evaluated once up front), no collectives issued"},
           "library_source_hash": library_source_hash(), "per_world": rows}
    finish(out)
    return 0


def finish(out):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.destroy_process_group()
    if out is not None:
        # the JSON line must be the last line of stdout: RCCL writes its version banner through C stdio, which would
        # otherwise be flushed at exit, after Python's own output
        import ctypes
        try:
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        sys.stdout.flush()
        print(json.dumps(out), flush=True)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--molecule", default="N2")
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--shard", choices=["batches", "rows"], default="batches",
                    help="batches: independent batches per rank (weak scaling, default); rows: ONE table, rows sharded over "
                         "the ranks, all-gather of log psi + all-reduce of the accumulators per step (strong scaling)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: kernel-duration brackets in the timed region and "
                         "`roofline`, `serial`, `config4_row_sharded`, `train_step`, `cpu_baseline` (the --no-* options "
                         "below leave parts of it out)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last one returned (log psi, E_loc, weighted sums) as "
                         "DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-serial-segment", action="store_true",
                    help="skip the one-batch-at-a-time segment that precedes the timed region (`serial`, `roofline.isolated`)")
    ap.add_argument("--no-train-step", action="store_true",
                    help="skip the training-step probe that follows the timed region (`train_step`: ms per VMC step of N2 / H2O / Li2O)")
    ap.add_argument("--no-config4", action="store_true",
                    help="skip the secondary row-sharded Li2O 50 000 table that follows the timed region (`config4_row_sharded`)")
    ap.add_argument("--emulate-world", default=None, metavar="W[,W...]",
                    help="scaling model without the node: on ONE GPU, time rank 0's share of the row-sharded table (log psi for "
                         "ceil(M/W) rows, E_loc for its rows against the whole table, no collectives) for every W given, e.g. "
                         "--emulate-world 1,2,4,8 --molecule Li2O --samples 50000; prints the implied strong-scaling ceiling")
    ap.add_argument("--pipeline", type=int, default=2,
                    help="independent batches in flight (HIP streams, one Hamiltonian/network handle pair each); 1 = serial")
    args = ap.parse_args(argv)
    if args.dump_outputs and args.emulate_world:
        ap.error("--dump-outputs: --emulate-world is a scaling model, it has no outputs of its own")
    return args


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    env_world = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and env_world is None:
        # the driver's convention `python bench.py --gpus N`: nobody started ranks for us -> start them ourselves,
        # before anything in this process touches the GPU
        return launch_ranks(args.gpus, argv)
    if env_world is not None and int(env_world) != args.gpus and int(os.environ.get("RANK", "0")) == 0:
        print(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={env_world} ranks; using {env_world}",
              file=sys.stderr)
    return worker(args)


if __name__ == "__main__":
    sys.exit(main())
