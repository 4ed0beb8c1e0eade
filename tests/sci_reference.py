"""The reference of selected CI (a plain helper module, like pt2_reference.py): the selection rule of
include/naqs_hip.h: naqs_ham_pt2_select restated in NumPy, operation for operation, and the loop of
DevicePauliHamiltonian.selected_ci with dense float64 blocks and numpy.linalg.eigh.

* ``importance``  eps, the intruder flags and the eligible flags of a set of rows;
* ``select``      the rule: -> (selected keys in row order, (count, intruders among them), dict(eps, eligible, tau, cut, mask));
* ``block``       H[rows, cols] of a packed Hamiltonian for two key lists, from the definition (no sector-wide matrix: N2's sector
                  has 14 400 states, its connected sets a few thousand);
* ``loop``        the iterations: eigh on S_t, the connected set (pt2_reference.connected_set), num = H[A, S] c and diag = H_aa,
                  E_PT2 over den > 0, ``select`` on (A ascending, num, diag), S_{t+1} = cat(S_t, selected);
* ``schedule``    n_add -> the k of each growth step and the number of iterations, as selected_ci reads it;
* ``start``       the determinant of lowest diagonal energy of a fixture's sector (a start that needs no eigenvector).
"""
import math
from functools import lru_cache

import numpy as np

import pt2_reference as ref


def importance(num, diag, e0, eps_min=0.0):
    num, diag = np.asarray(num, np.float64), np.asarray(diag, np.float64)
    with np.errstate(all="ignore"):
        den = diag - np.float64(e0)
        intruder = ~(den > 0) | np.isnan(num)
        eps = np.where(intruder, np.inf, (num * num) / den)
        eligible = (eps > 0) & (eps >= np.float64(eps_min))
    return eps, intruder, eligible


def select(keys, num, diag, e0, k, eps_min=0.0, tie_rtol=1e-9):
    keys = np.asarray(keys)
    eps, intruder, eligible = importance(num, diag, e0, eps_min)
    n_el = int(eligible.sum())
    tau = cut = None
    if k <= 0 or n_el == 0:
        mask = np.zeros(len(keys), bool)
    elif k >= n_el:
        mask = eligible.copy()
    else:
        tau = np.sort(eps[eligible])[n_el - k]
        with np.errstate(all="ignore"):
            cut = tau * np.float64(1.0 - tie_rtol)
            mask = eligible & (eps >= cut)
    return keys[mask], (int(mask.sum()), int((mask & intruder).sum())), dict(eps=eps, eligible=eligible, tau=tau, cut=cut, mask=mask)


def _parity(x):
    x = x.copy()
    for s in (32, 16, 8, 4, 2, 1):
        x ^= x >> np.uint64(s)
    return (x & np.uint64(1)).astype(np.int64)


def block(packed, rows, cols):
    """H[rows, cols]: entry (i, j) = sum over the terms with rows_i ^ xy == cols_j of coeff (-1)^popcount(rows_i & yz)."""
    rows, cols = np.asarray(rows, np.uint64), np.asarray(cols, np.uint64)
    order = np.argsort(cols)
    sorted_cols = cols[order]
    out = np.zeros((len(rows), len(cols)))
    if len(rows) == 0 or len(cols) == 0:
        return out
    at = np.arange(len(rows))
    for xy, yz, cf in zip(packed.xy, packed.yz, packed.coeff):
        j = rows ^ np.uint64(xy)
        pos = np.minimum(np.searchsorted(sorted_cols, j), len(cols) - 1)
        ok = sorted_cols[pos] == j
        sign = 1.0 - 2.0 * _parity(rows & np.uint64(yz))
        np.add.at(out, (at[ok], order[pos[ok]]), cf * sign[ok])
    return out


def diagonal(packed, rows):
    rows = np.asarray(rows, np.uint64)
    out = np.zeros(len(rows))
    for xy, yz, cf in zip(packed.xy, packed.yz, packed.coeff):
        if xy == 0:
            out += cf * (1.0 - 2.0 * _parity(rows & np.uint64(yz)))
    return out


def schedule(n_add):
    n_add = tuple(n_add)
    if len(n_add) == 2 and isinstance(n_add[1], float):
        return None, float(n_add[1]), int(n_add[0])
    return [int(k) for k in n_add], None, len(n_add) + 1


def loop(packed, keys0, n_add, eps_min=0.0, tie_rtol=1e-9):
    """-> dict(keys, vec, history=[dict(M, e0, e_pt2, n_external, n_intruders, n_added, k, eps, tau, cut)], stopped)."""
    ks, grow, n_iter = schedule(n_add)
    S = np.asarray(keys0, np.uint64).copy()
    Hss = block(packed, S, S)
    history, stopped, c = [], "schedule", None
    for t in range(n_iter):
        w, v = np.linalg.eigh(Hss)
        e0, c = float(w[0]), v[:, 0]
        A = ref.connected_set(packed, S)
        Has = block(packed, A, S)
        num, diag = Has @ c, diagonal(packed, A)
        eps, intruder, _ = importance(num, diag, e0)
        rec = dict(M=len(S), e0=e0, e_pt2=float(-np.sum(eps[~intruder])), n_external=len(A), n_intruders=int(intruder.sum()), n_added=0,
                   k=None, eps=eps, tau=None, cut=None)
        history.append(rec)
        if len(A) == 0:
            stopped = "connected set empty"
            break
        if t == n_iter - 1:
            break
        k = ks[t] if grow is None else int(math.ceil(grow * len(S)))
        sel, (n_sel, _), info = select(A, num, diag, e0, k, eps_min, tie_rtol)
        rec.update(k=k, tau=info["tau"], cut=info["cut"])
        if n_sel == 0:
            stopped = "nothing eligible"
            break
        rec["n_added"] = n_sel
        pick = info["mask"]
        Hnew = block(packed, sel, sel)
        Hss = np.block([[Hss, Has[pick].T], [Has[pick], Hnew]])
        S = np.concatenate([S, sel])
    return dict(keys=S, vec=c, history=history, stopped=stopped)


def cuts_are_clear(history, group_rtol=1e-12, clear_rtol=1e-6):
    """The schedules' precondition: at every cut no importance lies within clear_rtol (relative) of the cut, apart from the
    group within group_rtol of tau.  -> list of (iteration, offending eps) — empty when the precondition holds."""
    bad = []
    for t, h in enumerate(history):
        if h["cut"] is None:
            continue
        eps = h["eps"][np.isfinite(h["eps"]) & (h["eps"] > 0)]
        group = np.abs(eps - h["tau"]) <= group_rtol * h["tau"]
        near = np.abs(eps - h["cut"]) <= clear_rtol * h["cut"]
        bad += [(t, float(e)) for e in eps[near & ~group]]
    return bad


@lru_cache(maxsize=None)
def start(name):
    """-> (packed, fci energy, the sector's determinant of lowest H_aa as a one-key array)."""
    import os
    from conftest import GOLDEN
    from naqs_amd import packing
    path = os.path.join(GOLDEN, f"ham_{name}.npz")
    packed = packing.load_packed(path)
    with np.load(path) as z:
        fci = float(z["fci_energy"])
    keys = ref.sector_keys(packed.n_qubits, packed.n_alpha, packed.n_beta)
    return packed, fci, keys[[int(np.argmin(diagonal(packed, keys)))]]


# The schedules tests/test_sci_gpu.py runs on the device; tests/test_sci.py checks their precondition on the CPU.
SCHEDULES = {
    "LiH": (1, 2, 4, 8, 16, 32),
    "H2O": (1, 2, 4, 8, 16, 32),
    "N2": (1, 2, 4, 8, 16, 32, 64, 128),
}
