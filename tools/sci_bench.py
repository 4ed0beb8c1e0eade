"""Selected CI on one MI355X: what `naqs_ham_pt2_select` costs and what the loop gains.  One JSON line per figure.

    python tools/sci_bench.py time     [--reps 20]      (a) the kernel, both forms, against a torch composition of the same rule
    python tools/sci_bench.py sweep    [--reps 20]          both forms over n_ext = 2^9 .. 2^20 (and 10 240, 12 288, 14 336): where the crossover lies
    python tools/sci_bench.py converge                  (b) selected_ci from one determinant on LiH, H2O and N2
    python tools/sci_bench.py network  [--steps 300]        N2: a short training, then -sci from the network's own sample

(a) The rows: N2's external sets at the M = 100, 300, 1 500 and 10^4 determinants of largest coefficient (as tools/pt2_bench.py
builds them; num and diag from `pt2(rows=True)`), k = a quarter of the set, and synthetic rows (log-normal num and den, one row in
64 an intruder) at 10^6 and 10^7, k = a tenth.  Timed with HIP events around `reps` back-to-back calls after five warm-up calls,
in three rounds alternating: form 1 (one workgroup), form 2 (multi), the baseline.  The baseline is the rule from tensor ops: eps
by element-wise kernels, `torch.topk` for tau, the mask, `nonzero` (which reads the count back, as any host-sized result must; the
kernel's calls read nothing back).  Its selection is checked against the kernel's before anything is timed.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "naqs-for-quantum-chemistry_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _timed(fn, reps):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def _ham(mol):
    from naqs_amd import hamiltonian, packing
    path = os.path.join(GOLDEN, f"ham_{mol}.npz")
    packed = packing.load_packed(path)
    return packed, hamiltonian.DevicePauliHamiltonian(packed), float(np.load(path)["fci_energy"])


def torch_rule(keys, num, diag, e0, k, eps_min=0.0, tie_rtol=1e-9):
    """The rule from tensor ops (k below the number of eligible rows, as every timed case has it)."""
    den = diag - e0
    intr = ~(den > 0) | num.isnan()
    eps = torch.where(intr, torch.full_like(num, float("inf")), num * num / den)
    elig = (eps > 0) & (eps >= eps_min)
    tau = torch.topk(torch.where(elig, eps, torch.full_like(eps, -1.0)), k).values[-1]
    mask = elig & (eps >= tau * (1.0 - tie_rtol))
    return keys[mask.nonzero().squeeze(1)]


def synthetic(n, device, seed=0):
    gen = torch.Generator(device=device).manual_seed(seed)
    num = torch.randn(n, dtype=torch.float64, device=device, generator=gen).exp()
    den = torch.randn(n, dtype=torch.float64, device=device, generator=gen).exp()
    den[::64] = -1.0
    keys = torch.randperm(n, device=device, generator=gen).to(torch.int64) * 3 + 5
    return keys, num, den, 0.0


def n2_sets(ham, rows):
    import pt2_reference as ref
    from naqs_amd import hamiltonian
    p = ham.packed
    sector = ref.sector_keys(p.n_qubits, p.n_alpha, p.n_beta)
    all_d = hamiltonian.keys_to_device(sector, ham.device)
    e_full, v_full = ham.lowest_eigenpair(all_d, tol=1e-11)
    order = torch.argsort(v_full.abs(), descending=True)
    for M in rows:
        kd = all_d[order[:M]].contiguous()
        e_s, c = ham.lowest_eigenpair(kd, tol=1e-11)
        ext, n_ext = ham.connected_keys(kd)
        out4, num, diag = ham.pt2(kd, c, e_s, ext, rows=True)
        yield f"N2 M={M}", ext, num, diag, e_s


def time_case(ham, lib, name, keys, num, diag, e0, k, reps, forms=(1, 2), baseline=True):
    import ctypes
    from naqs_amd import _lib
    n = keys.shape[0]
    out = torch.empty(n, dtype=torch.int64, device=ham.device)
    count = torch.empty(2, dtype=torch.int64, device=ham.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel():
        _lib.check(lib.naqs_ham_pt2_select(ham._h, n, keys.data_ptr(), num.data_ptr(), diag.data_ptr(), e0, k, 0.0, 1e-9, n, out.data_ptr(),
                                           count.data_ptr(), stream), "naqs_ham_pt2_select")

    want = torch_rule(keys, num, diag, e0, k)
    for f in forms:
        os.environ["NAQS_SELECT_FORM"] = str(f)
        out.fill_(-1)
        kernel()
        n_sel = int(count[0])
        assert n_sel == want.shape[0] and torch.equal(out[:n_sel], want), (name, f, n_sel, want.shape[0])
    rounds = {f: [] for f in forms}
    base = []
    for _ in range(3):
        for f in forms:
            os.environ["NAQS_SELECT_FORM"] = str(f)
            rounds[f].append(round(_timed(kernel, reps), 2))
        if baseline:
            base.append(round(_timed(lambda: torch_rule(keys, num, diag, e0, k), reps), 2))
    os.environ.pop("NAQS_SELECT_FORM", None)
    print(json.dumps(dict(case=name, n_ext=n, k=k, selected=int(want.shape[0]), one_us=rounds.get(1), multi_us=rounds.get(2),
                          **(dict(torch_us=base) if baseline else {}), reps=reps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["time", "sweep", "converge", "network"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=300)
    args = ap.parse_args()
    from naqs_amd import _lib
    lib = _lib.load_library()
    if args.what == "time":
        packed, ham, fci = _ham("N2")
        for name, ext, num, diag, e_s in n2_sets(ham, (100, 300, 1500, 10000)):
            if ext.shape[0] >= 8:
                time_case(ham, lib, name, ext, num, diag, e_s, max(1, ext.shape[0] // 4), args.reps)
            else:
                print(json.dumps(dict(case=name, n_ext=int(ext.shape[0]), note="the table holds the whole block: nothing to select")), flush=True)
        for n in (10 ** 6, 10 ** 7):
            keys, num, diag, e0 = synthetic(n, ham.device)
            time_case(ham, lib, f"synthetic {n}", keys, num, diag, e0, n // 10, args.reps)
    elif args.what == "sweep":
        packed, ham, fci = _ham("LiH")
        for n in sorted([1 << b for b in range(9, 21)] + [10240, 12288, 14336]):
            keys, num, diag, e0 = synthetic(n, ham.device, seed=n % 97)
            time_case(ham, lib, f"synthetic {n}", keys, num, diag, e0, n // 10, args.reps, baseline=False)
    elif args.what == "converge":
        import sci_reference as sci
        from naqs_amd import hamiltonian
        for mol, n_iter in (("LiH", 8), ("H2O", 10), ("N2", 12)):
            packed, ham, fci = _ham(mol)
            k0 = sci.start(mol)[2]
            res = ham.selected_ci(hamiltonian.keys_to_device(k0, ham.device), (n_iter, 1.0), tol=1e-12)
            for h in res["history"]:
                print(json.dumps(dict(molecule=mol, M=h["M"], n_external=h["n_external"], n_added=h["n_added"], e_s_err=h["e0"] - fci,
                                      e_s_pt2_err=h["e0"] + h["e_pt2"] - fci, n_intruders=h["n_intruders"])), flush=True)
            print(json.dumps(dict(molecule=mol, stopped=res["stopped"], extrapolated_err=None if res["extrapolated"] is None
                                  else res["extrapolated"] - fci, kernel=ham.last_kernel())), flush=True)
    else:
        import tempfile
        from experiments import _base
        with tempfile.TemporaryDirectory() as tmp:
            res = _base.run(n_hid=64, argv=["-m", os.path.join(GOLDEN, "ham_N2.npz"), "-single_phase", "-n_hid", "64", "-n_hid_phase", "512",
                                            "-n_layer_phase", "2", "-n_samps", "1000000", "-n_unq_samps_min", "100", "-n_unq_samps_max",
                                            "100000", "-n_train", str(args.steps), "-output_freq", "100", "-s", "7", "-o", tmp, "-pt2",
                                            "-sci", "5"])
            r = res[0]
            print(json.dumps(dict(molecule="N2", steps=args.steps, final=r["final"], fci=r["fci"], n_unq=r["n_unq"], stopped=r["sci_stopped"],
                                  history=[dict(M=h["M"], n_external=h["n_external"], e_s_err=h["e0"] - r["fci"],
                                                e_s_pt2_err=h["e0"] + h["e_pt2"] - r["fci"]) for h in r["sci_history"]],
                                  extrapolated_err=None if r["sci_extrapolated"] is None else r["sci_extrapolated"] - r["fci"])), flush=True)


if __name__ == "__main__":
    main()
