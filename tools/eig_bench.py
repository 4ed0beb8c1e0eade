"""The two eigensolvers of `lowest_eigenpair` on one MI355X, on N2 subspaces a user would run: what a
diagonalisation costs with `solver="lanczos"` (the default, the tensor-op Lanczos) and with `solver="davidson"`
(`naqs_ham_eig_lowest`).  One JSON line per figure; both solvers alternate inside one process, three rounds.

    python tools/eig_bench.py [--reps 3] [--mode single | roots | gate] [--trace kernel_trace.csv]

* `cold`: the M = 100, 500, 1 500 and 10^4 determinants of largest coefficient in N2's ground state (tools/sci_bench.py's
  set-ups), each solver from the same seeded random start at tol 1e-10;
* `warm`: the subspaces of the committed selected-CI schedule (tests/sci_reference.py: SCHEDULES["N2"]), each from (c of the
  previous subspace, 0) at tol 1e-13, as `selected_ci` runs them;
* `loop`: the whole `selected_ci` run of that schedule with each solver.

Per call: wall time with a host clock around a call that ends in a synchronise (the median of `reps` calls after one warm-up
call), the products, the library's launches per product (`naqs_launch_count`; torch's own launches of the Lanczos path are not
counted by it), and the energy difference between the solvers.

`--mode roots`, on the same top-M subspaces of N2 (M = 100, 1 500, 10^4), alternating in one process, three rounds:
* `product`: one `block_product` of nb = 2, 4, 8 vectors against nb calls of `pt2` with the table's own keys as rows — the
  parent's product, `pt2_kernel`; both build the key table per call, `pt2` also runs its sums kernel, so these wall times bound
  the gain from above and `--mode gate` under a kernel trace gives the kernels' own times;
* `solver`: `lowest_eigenpairs` at k = 1, 2, 4 and, next to k = 1, `lowest_eigenpair(solver="davidson")`: wall time, products.
`--mode gate`: only the alternating products at M = 10^4, for a run under `rocprofv3 --kernel-trace --output-format csv`;
`--trace FILE` then reads that trace: per round, nb times the median `pt2_kernel` dispatch against the median `block_kernel`
dispatch plus its `block_pack_kernel`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "naqs-for-quantum-chemistry_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SOLVERS = ("lanczos", "davidson")


def timed_call(ham, lib, kd, reps, **kw):
    """-> (median wall time in us, products, library launches per product, energy)"""
    ham.lowest_eigenpair(kd, **kw)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        n0 = lib.naqs_launch_count()
        t0 = time.perf_counter()
        e, vec = ham.lowest_eigenpair(kd, **kw)
        torch.cuda.synchronize()
        times.append(1e6 * (time.perf_counter() - t0))
        launches = lib.naqs_launch_count() - n0
    products = ham.last_lanczos_iterations
    return round(float(np.median(times)), 1), products, round(launches / products, 2), e


def compare(ham, lib, name, kd, reps, **kw):
    rounds = {s: [] for s in SOLVERS}
    seen = {}
    for _ in range(3):
        for s in SOLVERS:
            us, products, per, e = timed_call(ham, lib, kd, reps, solver=s, **kw)
            rounds[s].append(us)
            seen[s] = (products, per, e)
    print(json.dumps(dict(case=name, M=int(kd.shape[0]), lanczos_us=rounds["lanczos"], davidson_us=rounds["davidson"],
                          lanczos_products=seen["lanczos"][0], davidson_products=seen["davidson"][0],
                          lanczos_lib_launches_per_product=seen["lanczos"][1], davidson_lib_launches_per_product=seen["davidson"][1],
                          energy_difference=seen["davidson"][2] - seen["lanczos"][2], kernel=ham.last_kernel(), reps=reps)), flush=True)


NBS = (2, 4, 8)


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


def products(ham, name, kd, reps):
    """Per round and nb: nb single products (pt2 on the table's own keys), then one block product of the same vectors."""
    M = int(kd.shape[0])
    gen = torch.Generator(device=ham.device).manual_seed(1)
    C = torch.randn((8, M), dtype=torch.float64, device=ham.device, generator=gen)
    single = {nb: [] for nb in NBS}
    block = {nb: [] for nb in NBS}
    for _ in range(3):
        for nb in NBS:
            single[nb].append(wall(lambda: [ham.pt2(kd, C[c], -1e3, kd) for c in range(nb)], reps))
            block[nb].append(wall(lambda: ham.block_product(kd, C[:nb]), reps))
    num, diag = ham.block_product(kd, C)
    same = all(torch.equal(num[c], ham.pt2(kd, C[c], -1e3, kd, rows=True)[1]) for c in range(8))
    print(json.dumps(dict(case=f"product, {name}", M=M, single_us={str(nb): single[nb] for nb in NBS},
                          block_us={str(nb): block[nb] for nb in NBS}, same_bits=same, kernel=ham.last_kernel(), reps=reps)), flush=True)


def solvers(ham, name, kd, reps):
    rounds = {k: [] for k in ("single", 1, 2, 4)}
    seen = {}
    for _ in range(3):
        rounds["single"].append(wall(lambda: ham.lowest_eigenpair(kd, solver="davidson", tol=1e-10), reps))
        seen["single"] = ham.last_eig_info["products"]
        for k in (1, 2, 4):
            rounds[k].append(wall(lambda: ham.lowest_eigenpairs(kd, k, tol=1e-10, m_max=16 if k == 1 else 32), reps))
            seen[k] = (ham.last_eig_info["products"], ham.last_eig_info["status"], [float(e) for e in ham.lowest_eigenpairs(kd, k, tol=1e-10)[0]])
    print(json.dumps(dict(case=f"solver, {name}", M=int(kd.shape[0]), eig_lowest_us=rounds["single"], eig_lowest_products=seen["single"],
                          **{f"k{k}_us": rounds[k] for k in (1, 2, 4)}, **{f"k{k}_products": seen[k][0] for k in (1, 2, 4)},
                          **{f"k{k}_status": seen[k][1] for k in (1, 2, 4)}, theta=seen[4][2], reps=reps)), flush=True)


def read_trace(path, reps):
    """The gate from a kernel trace of `--mode gate --reps reps`: dispatches in time order, three rounds of (nb: reps + 1 times nb
    pt2_kernel, reps + 1 times one block_pack_kernel + block_kernel) for nb = 2, 4, 8; the first call of each group is its warm-up."""
    import csv
    rows = sorted(((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                   for r in csv.DictReader(open(path))), key=lambda r: r[0])
    pt2 = [us for _, n, us in rows if "pt2_kernel" in n]
    blk = [us for _, n, us in rows if "block_kernel" in n]
    pack = [us for _, n, us in rows if "block_pack_kernel" in n]
    calls = reps + 1
    # (behind the rounds come the dispatches of the run's bit-for-bit check: 8 pt2_kernel, one block_kernel)
    assert len(pt2) == 3 * sum(NBS) * calls + 8 and len(blk) == len(pack) == 3 * len(NBS) * calls + 1, (len(pt2), len(blk), len(pack))
    out = {str(nb): dict(single_us=[], block_us=[]) for nb in NBS}
    i = j = 0
    for _ in range(3):
        for nb in NBS:
            one = pt2[i + nb:i + nb * calls]                       # (less the warm-up call's nb dispatches)
            i += nb * calls
            both = [a + b for a, b in zip(blk[j + 1:j + calls], pack[j + 1:j + calls])]
            j += calls
            out[str(nb)]["single_us"].append(round(nb * float(np.median(one)), 2))
            out[str(nb)]["block_us"].append(round(float(np.median(both)), 2))
    for nb in NBS:
        o = out[str(nb)]
        o["parent_spread_us"] = round(max(o["single_us"]) - min(o["single_us"]), 2)
        o["gain_us"] = round(float(np.median(o["single_us"]) - np.median(o["block_us"])), 2)
    print(json.dumps(dict(case="gate, kernel times from the trace", **out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mode", choices=["single", "roots", "gate"], default="single")
    ap.add_argument("--trace", default=None)
    args = ap.parse_args()
    if args.trace:
        return read_trace(args.trace, args.reps)
    import pt2_reference as ref
    import sci_reference as sci
    from naqs_amd import _lib, hamiltonian
    from sci_bench import _ham
    lib = _lib.load_library()
    packed, ham, fci = _ham("N2")
    sector = ref.sector_keys(packed.n_qubits, packed.n_alpha, packed.n_beta)
    all_d = hamiltonian.keys_to_device(sector, ham.device)
    e_full, v_full = ham.lowest_eigenpair(all_d, tol=1e-11)
    order = torch.argsort(v_full.abs(), descending=True)
    if args.mode == "gate":
        return products(ham, "N2 top 10000", all_d[order[:10000]].contiguous(), args.reps)
    if args.mode == "roots":
        for M in (100, 1500, 10000):
            products(ham, f"N2 top {M}", all_d[order[:M]].contiguous(), args.reps)
        for M in (100, 1500, 10000):
            solvers(ham, f"N2 top {M}", all_d[order[:M]].contiguous(), args.reps)
        return
    for M in (100, 500, 1500, 10000):
        compare(ham, lib, f"cold, N2 top {M}", all_d[order[:M]].contiguous(), args.reps, tol=1e-10)

    k0 = hamiltonian.keys_to_device(sci.start("N2")[2], ham.device)
    schedule = sci.SCHEDULES["N2"]
    grown = ham.selected_ci(k0, schedule, tol=1e-13)
    sizes = [h["M"] for h in grown["history"]]
    for small, large in zip(sizes, sizes[1:]):
        c = ham.lowest_eigenpair(grown["keys"][:small].contiguous(), tol=1e-13)[1]
        v0 = torch.cat([c, torch.zeros(large - small, dtype=torch.float64, device=ham.device)])
        compare(ham, lib, f"warm, schedule {small} -> {large}", grown["keys"][:large].contiguous(), args.reps, tol=1e-13, v0=v0)

    loop = {s: [] for s in SOLVERS}
    last = {}
    for _ in range(3):
        for s in SOLVERS:
            ham.selected_ci(k0, schedule, tol=1e-13, solver=s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[s] = ham.selected_ci(k0, schedule, tol=1e-13, solver=s)
            torch.cuda.synchronize()
            loop[s].append(round(1e3 * (time.perf_counter() - t0), 2))
    print(json.dumps(dict(case="loop, selected_ci on the N2 schedule", iterations=len(sizes), final_M=sizes[-1], lanczos_ms=loop["lanczos"],
                          davidson_ms=loop["davidson"],
                          worst_energy_difference=max(abs(a["e0"] - b["e0"]) for a, b in zip(last["lanczos"]["history"], last["davidson"]["history"])))),
          flush=True)


if __name__ == "__main__":
    main()
