"""The two eigensolvers of `lowest_eigenpair` on one MI355X, on N2 subspaces a user would run: what a
diagonalisation costs with `solver="lanczos"` (the default, the tensor-op Lanczos) and with `solver="davidson"`
(`naqs_ham_eig_lowest`).  One JSON line per figure; both solvers alternate inside one process, three rounds.

    python tools/eig_bench.py [--reps 3]

* `cold`: the M = 100, 500, 1 500 and 10^4 determinants of largest coefficient in N2's ground state (tools/sci_bench.py's
  set-ups), each solver from the same seeded random start at tol 1e-10;
* `warm`: the subspaces of the committed selected-CI schedule (tests/sci_reference.py: SCHEDULES["N2"]), each from (c of the
  previous subspace, 0) at tol 1e-13, as `selected_ci` runs them;
* `loop`: the whole `selected_ci` run of that schedule with each solver.

Per call: wall time with a host clock around a call that ends in a synchronise (the median of `reps` calls after one warm-up
call), the products, the library's launches per product (`naqs_launch_count`; torch's own launches of the Lanczos path are not
counted by it), and the energy difference between the solvers.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
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
