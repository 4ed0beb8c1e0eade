"""Selected CI for several roots on one MI355X: what one walk over the external rows saves, and what the loop costs.
One JSON line per figure.

    python tools/sci_roots_bench.py gate [--reps 5]      the alternating calls, for a run under a kernel trace
    python tools/sci_roots_bench.py --trace kernel_trace.csv [--reps 5]      the gate's kernel times from that trace
    python tools/sci_roots_bench.py wall [--reps 5]      the calls' wall times, and selected_ci_roots at K = 4

The rows: N2, the 10^4 determinants of largest coefficient of the sector's ground state and their connected set (as
tools/pt2_bench.py and tools/eig_bench.py build them); the vectors are seeded random rows, the energies lie below every H_aa.
`gate`: for nb = 2, 4, 8, three rounds alternating in one process: reps + 1 times nb calls of `naqs_ham_pt2` (the parent's route:
per call a key-table build, pt2_kernel, pt2_sums_kernel), then reps + 1 times one `naqs_ham_pt2_block` (one key-table build,
block_pack_kernel, block_kernel, pt2_block_sums_kernel); the first call of each group is its warm-up.  Run it as

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/sci_roots_bench.py gate

and hand the trace to `--trace`: per round nb x (median pt2_kernel + median pt2_sums_kernel) against the median of block_kernel +
block_pack_kernel + pt2_block_sums_kernel.  The key-table builds are left out of both sides (the parent's nb against one: the
comparison is the walk's and the sums').  The gate: at nb = 4 the gain exceeds the parent side's own spread over the rounds.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "naqs-for-quantum-chemistry_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

NBS = (2, 4, 8)


def rows_of_n2(M=10000):
    import pt2_reference as ref
    from naqs_amd import hamiltonian
    from sci_bench import _ham
    packed, ham, fci = _ham("N2")
    sector = ref.sector_keys(packed.n_qubits, packed.n_alpha, packed.n_beta)
    all_d = hamiltonian.keys_to_device(sector, ham.device)
    e_full, v_full = ham.lowest_eigenpair(all_d, tol=1e-11)
    kd = all_d[torch.argsort(v_full.abs(), descending=True)[:M]].contiguous()
    ext, n_ext = ham.connected_keys(kd)
    gen = torch.Generator(device=ham.device).manual_seed(1)
    C = torch.randn((8, M), dtype=torch.float64, device=ham.device, generator=gen)
    C /= C.norm(dim=1, keepdim=True)
    e = -1e3 + np.arange(8.0)
    return ham, kd, ext, C, e


def same_bits(ham, kd, ext, C, e):
    out4, num, diag = ham.pt2_block(kd, C, e, ext, rows=True)
    ok = True
    for c in range(8):
        w4, wn, wd = ham.pt2(kd, C[c], float(e[c]), ext, rows=True)
        ok = ok and torch.equal(num[c], wn) and torch.equal(diag, wd) and torch.equal(out4[c], w4)
    return ok


def wall(f, reps):
    f()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        times.append(1e6 * (time.perf_counter() - t0))
    return round(float(np.median(times)), 1)


def alternate(ham, kd, ext, C, e, reps):
    single = {nb: [] for nb in NBS}
    block = {nb: [] for nb in NBS}
    for _ in range(3):
        for nb in NBS:
            single[nb].append(wall(lambda: [ham.pt2(kd, C[c], float(e[c]), ext) for c in range(nb)], reps))
            block[nb].append(wall(lambda: ham.pt2_block(kd, C[:nb], e[:nb], ext), reps))
    return single, block


def read_trace(path, reps):
    """Dispatches in time order; the rounds are the run's last dispatches (the bit-for-bit check and the set-up come first)."""
    import csv
    rows = sorted(((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                   for r in csv.DictReader(open(path))), key=lambda r: r[0])
    calls = reps + 1

    def last(name, n):
        us = [t for _, k, t in rows if name in k]
        assert len(us) >= n, (name, len(us), n)
        return us[len(us) - n:]

    # a trace of `gate` and nothing else: the new sums kernel ran once in the bit-for-bit check and once per block call of the
    # rounds (a `wall` trace has the loop's dispatches behind them and would be misread)
    n_bsum = sum("pt2_block_sums_kernel" in k for _, k, _ in rows)
    assert n_bsum == 1 + 3 * len(NBS) * calls, f"not a trace of `gate --reps {reps}`: {n_bsum} pt2_block_sums_kernel dispatches"
    pt2 = last("pt2_kernel", 3 * sum(NBS) * calls)
    sums = last("pt2_sums_kernel", 3 * sum(NBS) * calls)
    blk, pack, bsum = (last(k, 3 * len(NBS) * calls) for k in ("block_kernel", "block_pack_kernel", "pt2_block_sums_kernel"))
    out = {str(nb): dict(single_us=[], block_us=[], walk_us=[], pack_us=[], sums_us=[]) for nb in NBS}
    i = j = 0
    for _ in range(3):
        for nb in NBS:
            one = float(np.median(pt2[i + nb:i + nb * calls])) + float(np.median(sums[i + nb:i + nb * calls]))      # (less the warm-up call)
            i += nb * calls
            parts = [float(np.median(x[j + 1:j + calls])) for x in (blk, pack, bsum)]
            both = float(np.median([a + b + c for a, b, c in zip(blk[j + 1:j + calls], pack[j + 1:j + calls], bsum[j + 1:j + calls])]))
            j += calls
            o = out[str(nb)]
            o["single_us"].append(round(nb * one, 2))
            o["block_us"].append(round(both, 2))
            for key, v in zip(("walk_us", "pack_us", "sums_us"), parts):
                o[key].append(round(v, 2))
    for nb in NBS:
        o = out[str(nb)]
        o["parent_spread_us"] = round(max(o["single_us"]) - min(o["single_us"]), 2)
        o["gain_us"] = round(float(np.median(o["single_us"]) - np.median(o["block_us"])), 2)
    out["gate_nb4_passed"] = bool(out["4"]["gain_us"] > out["4"]["parent_spread_us"])
    print(json.dumps(dict(case="gate, kernel times from the trace", **out)), flush=True)


def loop(reps):
    """selected_ci_roots at K = 4 on N2 from its four lowest determinants, the subspace doubling: wall time per iteration."""
    import sci_roots_reference as R
    from naqs_amd import hamiltonian
    from sci_bench import _ham
    packed, ham, fci = _ham("N2")
    k0 = hamiltonian.keys_to_device(R.start("N2", 4)[2], ham.device)
    n_iter = 10
    ham.selected_ci_roots(k0, 4, (n_iter, 1.0))
    torch.cuda.synchronize()
    total = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = ham.selected_ci_roots(k0, 4, (n_iter, 1.0))
        torch.cuda.synchronize()
        total.append(1e3 * (time.perf_counter() - t0))
    hist = res["history"]
    print(json.dumps(dict(case="loop, selected_ci_roots on N2, K = 4, grow 1.0", iterations=len(hist), M=[h["M"] for h in hist],
                          n_external=[h["n_external"] for h in hist], total_ms=[round(t, 2) for t in total],
                          ms_per_iteration=round(float(np.median(total)) / len(hist), 2), stopped=res["stopped"],
                          roots_minus_fci=[round(x - fci, 6) for x in res["eigs"]], kernel=ham.last_kernel())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", choices=["gate", "wall"], default="wall")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", default=None)
    args = ap.parse_args()
    if args.trace:
        return read_trace(args.trace, args.reps)
    ham, kd, ext, C, e = rows_of_n2()
    same = same_bits(ham, kd, ext, C, e)
    single, block = alternate(ham, kd, ext, C, e, args.reps)
    print(json.dumps(dict(case="pt2 rows and sums, N2 top 10000, wall", M=int(kd.shape[0]), n_ext=int(ext.shape[0]),
                          single_us={str(nb): single[nb] for nb in NBS}, block_us={str(nb): block[nb] for nb in NBS}, same_bits=same,
                          kernel=ham.last_kernel(), reps=args.reps)), flush=True)
    if args.what == "wall":
        loop(args.reps)


if __name__ == "__main__":
    main()
