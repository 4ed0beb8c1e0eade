"""The Epstein-Nesbet correction of a sampled-subspace energy on N2 (tests/golden/ham_N2.npz, 14 400 states in the sector): what it
gains and what it costs on one MI355X.  One JSON line per table size.

    python tools/pt2_bench.py [--rows 100,300,1500,10000] [--reps 20]

The table S: the M determinants of largest |coefficient| in the ground state, which the device Lanczos finds on the whole sector
(the largest draw there is); c, E_S: the device Lanczos on S.  The ground state lives in one symmetry block of the sector (the first
line printed counts the determinants whose coefficient is above 1e-10): a table of 1 500 is most of it and connects to the few hundred it lacks, a table
of 10^4 holds all of it, so its correction is zero to rounding and only its time is of interest; 100 and 300 show the gain.  Timed, HIP events around `reps` back-to-back calls after five
warm-up calls:
  connected   DevicePauliHamiltonian.connected_keys (naqs_ham_connected, the count read back, the sort)
  pt2         naqs_ham_pt2 over the connected set A
  baseline    the same rows from the entries the library had before: naqs_hmatvec on the union table S + A, rows [M, M + n_ext),
              v = (c, 0), and naqs_get_hij on A for the diagonals (column 0 of a dense n_ext x Kxy matrix)
pt2 and baseline alternate over three rounds in one process; each round's figure is printed.  The baseline's numerators are
checked against the new call's before anything is timed.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "naqs-for-quantum-chemistry_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100,300,1500,10000")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from naqs_amd import _lib, hamiltonian, packing
    import pt2_reference as ref
    path = os.path.join(ROOT, "tests", "golden", "ham_N2.npz")
    packed = packing.load_packed(path)
    fci = float(np.load(path)["fci_energy"])
    ham = hamiltonian.DevicePauliHamiltonian(packed)
    lib = _lib.load_library()
    sector = ref.sector_keys(packed.n_qubits, packed.n_alpha, packed.n_beta)
    all_d = hamiltonian.keys_to_device(sector, ham.device)
    e_full, v_full = ham.lowest_eigenpair(all_d, tol=1e-11)
    order = torch.argsort(v_full.abs(), descending=True)
    print(json.dumps(dict(molecule="N2", sector=len(sector), support=int((v_full.abs() > 1e-10).sum()), e_full_sector=e_full, fci=fci)),
          flush=True)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for M in (int(r) for r in args.rows.split(",")):
        kd = all_d[order[:M]].contiguous()
        e_s, c = ham.lowest_eigenpair(kd, tol=1e-11)
        ext, n_ext = ham.connected_keys(kd)
        res = ham.pt2_correction(kd, c, e0=e_s)
        out4, num, diag = ham.pt2(kd, c, e_s, ext, rows=True)
        name = ham.last_kernel()
        # the baseline and its check
        union = torch.cat([kd, ext]).contiguous()
        v = torch.zeros((M + n_ext, 2), dtype=torch.float64, device=ham.device)
        v[:M, 0] = c
        hv = torch.empty((n_ext, 2), dtype=torch.float64, device=ham.device)
        hij = torch.empty((n_ext, ham.Kxy), dtype=torch.float64, device=ham.device)

        def baseline():
            _lib.check(lib.naqs_hmatvec(ham._h, M + n_ext, union.data_ptr(), v.data_ptr(), M, n_ext, hv.data_ptr(), stream), "naqs_hmatvec")
            _lib.check(lib.naqs_get_hij(ham._h, n_ext, ext.data_ptr(), hij.data_ptr(), stream), "naqs_get_hij")

        sums = torch.empty(4, dtype=torch.float64, device=ham.device)

        def new():
            _lib.check(lib.naqs_ham_pt2(ham._h, M, kd.data_ptr(), c.data_ptr(), e_s, n_ext, ext.data_ptr(), None, None, sums.data_ptr(),
                                        stream), "naqs_ham_pt2")

        baseline()
        torch.cuda.synchronize()
        base_name = "eloc_kernel2" if "eloc_kernel2" in ham.last_kernel() else ham.last_kernel()
        err = float((hv[:, 0] - num).abs().max())
        err_d = float((hij[:, 0] - diag).abs().max())
        den = e_s - hij[:, 0]
        e_base = float((hv[:, 0] ** 2 / den)[den < 0].sum())
        assert err <= 1e-12 and err_d <= 1e-10 and abs(e_base - res["e_pt2"]) <= 1e-12, (err, err_d, e_base, res["e_pt2"])
        t_conn = _timed(lambda: ham.connected_keys(kd), args.reps)
        rounds = []
        for _ in range(3):
            rounds.append((_timed(new, args.reps), _timed(baseline, args.reps)))
        print(json.dumps(dict(molecule="N2", M=M, n_ext=n_ext, kernel=name, baseline_kernel=base_name, fci=fci, e_full_sector=e_full,
                              e_s=e_s, e_pt2=res["e_pt2"], e_s_err=e_s - fci, e_s_pt2_err=e_s + res["e_pt2"] - fci,
                              n_intruders=res["n_intruders"], connected_us=round(t_conn, 2),
                              pt2_us=[round(a, 2) for a, _ in rounds], baseline_us=[round(b, 2) for _, b in rounds],
                              max_abs_num_diff=err, max_abs_diag_diff=err_d, reps=args.reps)), flush=True)


if __name__ == "__main__":
    main()
