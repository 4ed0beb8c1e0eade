"""Exact local energies (naqs_ham_connected + log psi of the connected states + E_loc on table + connected states): N2 with 750
and 10^4 sampled rows, Li2O with 3 000, random-parameter networks of the published shape.  Per shape one JSON line: the size of
the connected set, connected_kernel's call (hipEvent brackets, prep + kernel, the host read of the count excluded), the whole
exact call next to the truncated call on the same table (wall time, synchronised).  Run under
`rocprofv3 --kernel-trace --stats -- python tools/exact_eloc_bench.py` for the kernel rows.

    python tools/exact_eloc_bench.py [--reps 20]

`train` mode — the training step on exact local energies (``PartialSamplingOptimizer(..., exact_local_energies=True)``) next to the
truncated step and to the route that existed before ``naqs_exact_eloc`` (``forward_saved`` + the Python evaluator of
``_exact_local_energy`` + ``backward_from_local_energy``), on one fixed table per shape: N2 at 750 and 1 400 rows, H2O at 300,
Li2O at 3 000.  The legs alternate in chunks inside one process after a warm-up, each on its own copy of the same network; the
old route runs twice and the gap between its two legs is the spread the new step is judged against.  One JSON line per shape,
also written to profiles/exact_train.txt (the tool's own file: nothing else is kept there).

    python tools/exact_eloc_bench.py train [--steps 200] [--chunk 20] [--out profiles/exact_train.txt]

`connected` mode — `naqs_ham_connected` with connected_kernel's per-wave append (NAQS_CONN_WG=0, two legs: their gap is the
spread) and its per-workgroup append (the default), alternating in one process at the three shapes above -> one JSON line per
shape, also written to profiles/exact_connected_ab.txt.

    python tools/exact_eloc_bench.py connected [--reps 20] [--ab-out profiles/exact_connected_ab.txt]
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

SHAPES = [("N2", 20, 7, 7, 750), ("N2", 20, 7, 7, 10000), ("Li2O", 30, 7, 7, 3000)]


def _opt(mol, N, na, nb, tmp):
    from naqs_amd import packing
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.optimizer import PartialSamplingOptimizer
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    hil = Hilbert.get(N, na, nb, encoding=Encoding.SIGNED)
    torch.manual_seed(1)
    wf = NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, amp_hidden_size=[64], phase_hidden_size=[512, 512],
                                   use_amp_spin_sym=True, use_phase_spin_sym=False, aggregate_phase=False,
                                   n_alpha_electrons=na, n_beta_electrons=nb)
    ham = packing.load_packed(os.path.join(ROOT, "tests", "golden", f"ham_{mol}.npz"))
    return PartialSamplingOptimizer(
        n_samples=1e6, n_samples_max=1e12, n_unq_samples_min=10, n_unq_samples_max=1e5, log_exact_energy=False, wavefunction=wf,
        qubit_hamiltonian=ham, pre_compute_H=False, n_electrons=na + nb, n_alpha_electrons=na, n_beta_electrons=nb,
        normalise_psi=True, grad_clip_factor=None, optimizer=torch.optim.Adam,
        optimizer_args=[{'lr': 1e-3, 'betas': (0.9, 0.99), 'weight_decay': 0, 'eps': 1e-15, 'amsgrad': False}, {'lr': 1e-2}],
        save_loc=tmp, pauli_hamiltonian_dtype=np.float64, seed=111)


def _wall_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def shape(mol, N, na, nb, rows, reps):
    import grad_reference as gr
    from naqs_amd import _lib
    from naqs_amd.hamiltonian import _stream_ptr
    with tempfile.TemporaryDirectory() as tmp:
        opt = _opt(mol, N, na, nb, tmp)
        ham = opt.pauli_hamiltonian
        keys = torch.as_tensor(gr.random_keys(opt.hilbert, rows, 3).astype(np.int64), device="cuda")
        conn, count = ham.connected_keys(keys)
        kernel = ham.last_kernel()
        # the library call alone: prep + connected_kernel, no read of the count in between
        cap = ham.connected_capacity(rows, rows)
        out = torch.empty(cap, dtype=torch.int64, device="cuda")
        cnt = torch.empty(1, dtype=torch.int64, device="cuda")
        lib = _lib.load_library()

        def call():
            _lib.check(lib.naqs_ham_connected(ham._h, rows, keys.data_ptr(), 0, rows, cap, out.data_ptr(), cnt.data_ptr(),
                                              _stream_ptr(ham.device)), "naqs_ham_connected")
        for _ in range(3):
            call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            call()
        b.record()
        torch.cuda.synchronize()
        lp = opt._log_psi_of_keys(keys)
        res = dict(what="exact E_loc", molecule=mol, rows=rows, n_connected=count, capacity=cap, kernel=kernel,
                   connected_call_us=1e3 * a.elapsed_time(b) / reps,
                   exact_ms=_wall_ms(lambda: opt.calculate_local_energy(keys, log_psi=lp, set_unsampled_states_to_zero=False), reps),
                   truncated_ms=_wall_ms(lambda: opt.calculate_local_energy(keys, log_psi=lp), reps),
                   logpsi_connected_ms=_wall_ms(lambda: opt._log_psi_of_keys(conn), reps) if count else 0.0)
        ham.local_energy(torch.cat([keys, conn]), torch.cat([lp, opt._log_psi_of_keys(conn)]), kind="log_psi", row_begin=0, n_rows=rows)
        res["eloc_kernel_on_the_union"] = ham.last_kernel()
    return res


TRAIN_SHAPES = [("N2", 20, 7, 7, 750), ("N2", 20, 7, 7, 1400), ("H2O", 14, 5, 5, 300), ("Li2O", 30, 7, 7, 3000)]


def _old_route_step(opt, keys, w):
    """The exact step as it could be written before naqs_exact_eloc: the same forward, backward and update, the local
    energies from the evaluation path (count read back, sort, two concatenations, a float64 copy, a second library call)."""
    wf = opt.wavefunction
    fused = wf.fused(need_phase=True)
    lp, saved = fused.forward_saved(keys)
    e, sums, _ = opt._exact_local_energy(keys, log_psi=lp, weights=w)
    opt.optimizer.zero_grad()
    g, ev = fused.backward_from_local_energy(saved, e, w, sums)
    opt.optimizer.step()
    wf.parameters_changed()
    wf.fused(need_phase=True)
    opt.optimizer.zero_grad()
    return ev


def train_shape(mol, N, na, nb, rows, steps, chunk):
    import grad_reference as gr
    from naqs_amd import _lib
    lib = _lib.load_library()
    with tempfile.TemporaryDirectory() as tmp:
        opts = {leg: _opt(mol, N, na, nb, os.path.join(tmp, leg)) for leg in ("truncated", "old_route_a", "old_route_b", "exact")}
        opts["exact"].exact_local_energies = True
        for o in opts.values():
            o.track_sampled_idxs = False
        keys = torch.as_tensor(gr.random_keys(opts["exact"].hilbert, rows, 3).astype(np.int64), device="cuda")
        w = torch.rand(rows, dtype=torch.float64, device="cuda") + 0.1
        w = (w / w.sum()).contiguous()
        run = {"truncated": lambda: opts["truncated"]._SGD_step(None, keys, None, sample_weights=w, lazy=True),
               "old_route_a": lambda: _old_route_step(opts["old_route_a"], keys, w),
               "old_route_b": lambda: _old_route_step(opts["old_route_b"], keys, w),
               "exact": lambda: opts["exact"]._SGD_step(None, keys, None, sample_weights=w, lazy=True)}
        for fn in run.values():                                   # warm-up: scratch, buffers, code objects
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        total = {leg: 0.0 for leg in run}
        launches = {leg: 0 for leg in run}
        done = 0
        while done < steps:
            for leg, fn in run.items():
                torch.cuda.synchronize()
                l0, t0 = lib.naqs_launch_count(), time.perf_counter()
                for _ in range(chunk):
                    fn()
                torch.cuda.synchronize()
                total[leg] += time.perf_counter() - t0
                launches[leg] += lib.naqs_launch_count() - l0
            done += chunk
        ms = {leg: 1e3 * t / done for leg, t in total.items()}
        # the library call of the exact step alone, synchronised on both sides: connected_kernel, the rendezvous, the forward
        # of the set, prep + E_loc over the union
        o = opts["exact"]
        fused, ham = o.wavefunction.fused(need_phase=True), o.pauli_hamiltonian
        cap = min(o.exact_max_table - rows, ham.connected_capacity(rows, rows))
        kbuf, lbuf = o._exact_buffers(rows + cap)
        kbuf[:rows].copy_(keys)
        fused.forward_saved(kbuf[:rows], out=lbuf[:rows])
        count = fused.exact_local_energy(ham, kbuf, lbuf, rows, 0, rows, cap, weights=w)[2]
        call_ms = _wall_ms(lambda: fused.exact_local_energy(ham, kbuf, lbuf, rows, 0, rows, cap, weights=w), 50)
        spread = abs(ms["old_route_a"] - ms["old_route_b"])
        old = min(ms["old_route_a"], ms["old_route_b"])
        return dict(what="exact training step", molecule=mol, rows=rows, n_connected=count, steps_per_leg=done,
                    truncated_ms=ms["truncated"], old_route_ms=[ms["old_route_a"], ms["old_route_b"]], old_route_spread_ms=spread,
                    exact_ms=ms["exact"], faster_outside_spread=bool(ms["exact"] < old - spread),
                    exact_call_alone_ms=call_ms, library_launches_per_step={leg: n / done for leg, n in launches.items()})


def connected_ab(mol, N, na, nb, rows, rounds, calls):
    """naqs_ham_connected (prep + connected_kernel, hipEvent brackets) with the per-wave append (twice: the spread) and the
    per-workgroup append (the default; NAQS_CONN_WG=1), alternating in one process; the sets compared."""
    import grad_reference as gr
    from naqs_amd import _lib
    from naqs_amd.hamiltonian import _stream_ptr
    with tempfile.TemporaryDirectory() as tmp:
        opt = _opt(mol, N, na, nb, tmp)
        ham = opt.pauli_hamiltonian
        keys = torch.as_tensor(gr.random_keys(opt.hilbert, rows, 3).astype(np.int64), device="cuda")
        cap = ham.connected_capacity(rows, rows)
        out = torch.empty(cap, dtype=torch.int64, device="cuda")
        cnt = torch.empty(1, dtype=torch.int64, device="cuda")
        lib = _lib.load_library()

        def call():
            _lib.check(lib.naqs_ham_connected(ham._h, rows, keys.data_ptr(), 0, rows, cap, out.data_ptr(), cnt.data_ptr(),
                                              _stream_ptr(ham.device)), "naqs_ham_connected")
        legs = [("per_wave_a", "0"), ("per_workgroup", "1"), ("per_wave_b", "0")]
        sets, kernels, us = {}, {}, {leg: 0.0 for leg, _ in legs}
        for leg, v in legs:
            os.environ["NAQS_CONN_WG"] = v
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            sets[leg] = torch.sort(out[:int(cnt.item())]).values.clone()
            kernels[leg] = ham.last_kernel()
        for _ in range(rounds):
            for leg, v in legs:
                os.environ["NAQS_CONN_WG"] = v
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(calls):
                    call()
                b.record()
                torch.cuda.synchronize()
                us[leg] += 1e3 * a.elapsed_time(b) / calls
        os.environ.pop("NAQS_CONN_WG", None)
        us = {leg: t / rounds for leg, t in us.items()}
        spread = abs(us["per_wave_a"] - us["per_wave_b"])
        return dict(what="connected_kernel append A/B", molecule=mol, rows=rows, n_connected=int(sets["per_wave_a"].numel()),
                    same_set=bool(torch.equal(sets["per_wave_a"], sets["per_workgroup"])), call_us=us, per_wave_spread_us=spread,
                    per_workgroup_faster_outside_spread=bool(us["per_workgroup"] < min(us["per_wave_a"], us["per_wave_b"]) - spread),
                    kernels=kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="eloc", choices=["eloc", "train", "connected"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_train.txt"))
    ap.add_argument("--ab-out", dest="ab_out", default=os.path.join(ROOT, "profiles", "exact_connected_ab.txt"))
    a = ap.parse_args()
    if a.mode == "train":
        lines = []
        for s in TRAIN_SHAPES:
            lines.append(json.dumps(train_shape(*s, a.steps, a.chunk)))
            print(lines[-1], flush=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.mode == "connected":
        lines = []
        for s in SHAPES:
            lines.append(json.dumps(connected_ab(*s, 10, a.reps)))
            print(lines[-1], flush=True)
        with open(a.ab_out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    for s in SHAPES:
        print(json.dumps(shape(*s, a.reps)), flush=True)


if __name__ == "__main__":
    main()
