"""The natural-gradient step (minSR, naqs_sr.hip) on the published ansatz: times of its library calls for one table of N2, and the
steps / wall time to an energy with the natural gradient and with Adam from the same seed.  One JSON line per measurement.

    python tools/sr_bench.py [--rows 1500,10000] [--reps 20]                  the calls of one step (HIP events around each call)
    python tools/sr_bench.py --converge LiH --target -7.8810 --max-steps 500  steps and seconds until <E> of a step <= target
                             [--sr-solver hip]                                with the library's Cholesky solve
                             [--sr-momentum 0.9]                              with SPRING's momentum

The calls: the training forward; naqs_net_sr_gram_uncentred (the factor kernels + sr_gram_kernel twice); naqs_net_sr_gram (the same
+ row sums and centring); the two float64 Cholesky solves, by torch and by naqs_net_sr_solve — measured alternately in the same
call, three rounds, each repetition on fresh copies of T because the solve overwrites it (the copies are outside the timed
region); naqs_net_sr_direction (seeds + the training backward); naqs_net_sr_jvp (the factor kernels + sr_jvp_kernel twice: the
call a step with momentum adds), alternately with naqs_net_sr_gram, three rounds.
sr_gram_kernel's share of the f64-MFMA peak is computed from the uncentred call (an upper bound of the kernel's time); run under
`rocprofv3 --kernel-trace --stats -- python tools/sr_bench.py --rows 1500` for the per-kernel split.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "naqs-for-quantum-chemistry_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_F64_MFMA = 78.6e12          # the MI355X data sheet's FP64 matrix figure (sr_gram_kernel runs v_mfma_f64_16x16x4_f64)
SECTOR = {"LiH": (12, 2, 2), "H2O": (14, 5, 5), "N2": (20, 7, 7)}


def _net(mol, seed=111):
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    N, na, nb = SECTOR[mol]
    hil = Hilbert.get(N, na, nb, encoding=Encoding.SIGNED, make_basis=True)
    torch.manual_seed(seed)
    wf = NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, amp_hidden_size=[64], phase_hidden_size=[512, 512],
                                   use_amp_spin_sym=True, aggregate_phase=False, n_alpha_electrons=na, n_beta_electrons=nb)
    return hil, wf


def _timed(fn, reps):
    for _ in range(2):
        out = fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps, out


def _timed_fresh(fn, fresh, reps):
    """Mean microseconds of fn(*fresh()) over reps calls, each on fresh arguments made outside the timed region."""
    fn(*fresh())
    torch.cuda.synchronize()
    total = 0.0
    for _ in range(reps):
        args = fresh()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(*args)
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
    return 1e3 * total / reps, out


def gram_flops(P, Ha, phase, M):
    """Multiply-adds x 2 of sr_gram_kernel's products over the upper triangle of 64 x 64 tiles (both blocks): per amplitude pair
    the depths 32 (d-out) + Ha (h) + Ha (d-pre) + 32 (x), per phase layer its padded output and input widths."""
    r32 = lambda v: (v + 31) // 32 * 32
    depth = P * (64 + 2 * r32(Ha))
    widths = [2 * (P - 1)] + list(phase) + [4]
    depth += sum(r32(widths[l]) + r32(widths[l + 1]) for l in range(len(widths) - 1))
    nt = (M + 63) // 64
    return 2.0 * depth * 64 * 64 * nt * (nt + 1) / 2


def step_calls(rows, reps):
    hil, wf = _net("N2")
    fused = wf.fused(need_phase=True)
    keys = np.sort(np.random.RandomState(0).permutation(hil.restricted2full_idx(np.arange(hil.size)))[:rows])
    kd = torch.as_tensor(keys.astype(np.int64), device="cuda")
    rs = np.random.RandomState(1)
    w = rs.random_sample(rows) + 0.1
    w = torch.as_tensor(w / w.sum(), device="cuda")
    e = rs.normal(-107.0, 1.0, rows)
    g = torch.as_tensor(np.stack([2 * w.cpu().numpy() * (e - (w.cpu().numpy() * e).sum()), rs.normal(0, 1e-4, rows)], -1),
                        dtype=torch.float32, device="cuda")
    t_fwd, (_, saved) = _timed(lambda: fused.forward_saved(kd), reps)
    t_unc, _ = _timed(lambda: fused.sr_gram(saved, None, None, None, uncentred=True), reps)
    t_gram, (Ta, Tp, ya, yp) = _timed(lambda: fused.sr_gram(saved, w, g, 1e-3), reps)

    def solves():
        return [torch.cholesky_solve(y.unsqueeze(1), torch.linalg.cholesky_ex(T)[0]).squeeze(1) for T, y in ((Ta, ya), (Tp, yp))]

    t_solve, (xa, xp) = _timed(solves, max(1, reps // 4))
    # the two solvers alternately, three rounds, every repetition on fresh copies of T (naqs_net_sr_solve overwrites it; torch's
    # path gets the same copies so that both are measured alike)
    from naqs_amd import _lib
    lib = _lib.load_library()
    fresh = lambda: (Ta.clone(), Tp.clone())
    torch_solves = lambda A, P: [torch.cholesky_solve(y.unsqueeze(1), torch.linalg.cholesky_ex(T)[0]).squeeze(1) for T, y in ((A, ya), (P, yp))]
    hip_solves = lambda A, P: fused.sr_solve(A, P, ya, yp)
    rounds_torch, rounds_hip = [], []
    for _ in range(3):
        rounds_torch.append(_timed_fresh(torch_solves, fresh, max(1, reps // 4))[0])
        t, (ha, hp, info) = _timed_fresh(hip_solves, fresh, max(1, reps // 4))
        rounds_hip.append(t)
    n0 = lib.naqs_launch_count()
    hip_solves(*fresh())
    solve_launches = lib.naqs_launch_count() - n0
    assert info.tolist() == [0, 0]
    solve_flops = 2.0 * (rows ** 3 / 3.0 + 2.0 * rows ** 2)
    hip_vs_torch = [float(((h - x).abs().max() / x.abs().max()).item()) for h, x in ((ha, xa), (hp, xp))]
    t_dir, _ = _timed(lambda: fused.sr_direction(saved, w, xa, xp), reps)
    # the momentum step's extra call (naqs_net_sr_jvp: the factor kernels + sr_jvp_kernel twice) alternately with the plain step's
    # own Gram call, three rounds in this one process
    v = torch.as_tensor(rs.normal(0, 1e-2, fused.n_params), dtype=torch.float32, device="cuda")
    rounds_jvp, rounds_gram = [], []
    for _ in range(3):
        rounds_gram.append(_timed(lambda: fused.sr_gram(saved, w, g, 1e-3), reps)[0])
        rounds_jvp.append(_timed(lambda: fused.sr_jvp(saved, v), reps)[0])
    n0 = lib.naqs_launch_count()
    fused.sr_jvp(saved, v)
    jvp_launches = lib.naqs_launch_count() - n0
    flops = gram_flops(hil.N // 2, 64, (512, 512), rows)
    return dict(what="N2 natural-gradient step, per call", rows=rows, us_forward=t_fwd, us_factors_and_gram=t_unc,
                us_gram_and_centring=t_gram, us_two_cholesky_solves=t_solve, us_direction=t_dir,
                us_two_cholesky_solves_rounds=rounds_torch, us_two_hip_solves_rounds=rounds_hip,
                us_two_hip_solves=float(np.median(rounds_hip)), hip_solve_launches=int(solve_launches),
                us_step_hip=t_fwd + t_gram + float(np.median(rounds_hip)) + t_dir,
                us_jvp=float(np.median(rounds_jvp)), us_jvp_rounds=rounds_jvp, us_gram_and_centring_rounds=rounds_gram,
                jvp_launches=int(jvp_launches),
                us_step_hip_with_momentum=t_fwd + t_gram + float(np.median(rounds_jvp)) + float(np.median(rounds_hip)) + t_dir, solve_gflop=solve_flops / 1e9,
                hip_solve_fraction_of_f64_mfma_peak=solve_flops / (float(np.median(rounds_hip)) * 1e-6) / PEAK_F64_MFMA,
                hip_vs_torch_max_rel_diff=hip_vs_torch,
                us_step=t_fwd + t_gram + t_solve + t_dir, gram_gflop=flops / 1e9,
                gram_fraction_of_f64_mfma_peak_lower_bound=flops / (t_unc * 1e-6) / PEAK_F64_MFMA)


def converge(mol, target, max_steps, natural_gradient, n_samples):
    from naqs_amd import packing
    from naqs_amd.optimizer import LogKey, PartialSamplingOptimizer
    N, na, nb = SECTOR[mol]
    hil, wf = _net(mol)
    ham = packing.load_packed(os.path.join(ROOT, "tests", "golden", f"ham_{mol}.npz"))
    with tempfile.TemporaryDirectory() as tmp:
        opt = PartialSamplingOptimizer(
            n_samples=n_samples, n_samples_max=1e12, n_unq_samples_min=10, n_unq_samples_max=1e5, log_exact_energy=False,
            wavefunction=wf, qubit_hamiltonian=ham, pre_compute_H=False, n_electrons=na + nb, n_alpha_electrons=na,
            n_beta_electrons=nb, normalise_psi=True, grad_clip_factor=None, optimizer=torch.optim.Adam,
            optimizer_args=[{'lr': 1e-3, 'betas': (0.9, 0.99), 'weight_decay': 0, 'eps': 1e-15, 'amsgrad': False}, {'lr': 1e-2}],
            save_loc=tmp, pauli_hamiltonian_dtype=np.float64, seed=111,
            **({"natural_gradient": natural_gradient} if natural_gradient else {}))
        torch.cuda.synchronize()
        t0, steps, reached, last = time.perf_counter(), 0, None, float("nan")
        while steps < max_steps and reached is None:
            opt.run(n_epochs=25, save_freq=None, save_final=False, output_freq=1)
            steps += 25
            for s, e in opt.log[LogKey.E_LOC][-25:]:
                last = float(e)
                if last <= target and reached is None:
                    reached = int(s)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return dict(what=f"{mol} steps to <E> <= {target}", optimiser="natural gradient" if natural_gradient else "adam",
                hyper=natural_gradient, reached_at_step=reached, steps_run=steps, seconds=dt, last_energy=last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1500,10000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--converge", default=None)
    ap.add_argument("--target", type=float, default=None)
    ap.add_argument("--max-steps", type=int, default=500)
    ap.add_argument("--n-samples", type=float, default=1e6)
    ap.add_argument("--sr-shift", type=float, default=1e-3)
    ap.add_argument("--sr-lr", type=float, default=0.1)
    ap.add_argument("--sr-solver", choices=["torch", "hip"], default=None)
    ap.add_argument("--sr-momentum", type=float, default=0.0)
    a = ap.parse_args()
    if a.converge:
        for ng in (dict(dict(diag_shift=a.sr_shift, lr=a.sr_lr), **({"solver": a.sr_solver} if a.sr_solver else {}),
                        **({"momentum": a.sr_momentum} if a.sr_momentum else {})), None):
            print(json.dumps(converge(a.converge, a.target, a.max_steps, ng, int(a.n_samples))), flush=True)
        return
    for rows in (int(r) for r in a.rows.split(",")):
        print(json.dumps(step_calls(rows, a.reps)), flush=True)


if __name__ == "__main__":
    main()
