"""The reference of selected CI for several roots (a plain helper module, like sci_reference.py, which it imports): the averaged
selection rule of include/naqs_hip.h: naqs_ham_pt2_select_avg restated in NumPy, operation for operation, and the loop of
DevicePauliHamiltonian.selected_ci_roots with dense float64 blocks and numpy.linalg.eigh.

* ``importance``  eps, the intruder flags and the eligible flags of a set of rows, num [nb, n];
* ``select``      the rule: -> (selected keys in row order, (count, intruders among them), dict(eps, eligible, tau, cut, mask));
* ``loop``        the iterations: eigh on S_t and its n_roots lowest pairs, the connected set (pt2_reference.connected_set),
                  num = (H[A, S] C)^T and diag = H_aa, every root's E_PT2 over its own den > 0, ``select`` on (A ascending, num,
                  diag), S_{t+1} = cat(S_t, selected);
* ``start``       the n_roots determinants of lowest diagonal energy of a fixture's sector;
* ``SCHEDULES_ROOTS``  what tests/test_sci_roots_gpu.py runs on the device; tests/test_sci_roots.py checks the preconditions.
"""
import math
from functools import lru_cache

import numpy as np

import pt2_reference as ref
import sci_reference as sci


def equal_weights(nb):
    return np.full(nb, 1.0 / nb)


def importance(num, diag, e, w, eps_min=0.0):
    """One float64 rounding per operation, as the header writes them: den_j = diag - e_j, q_j = (num_j * num_j) / den_j,
    eps = w_j0 * q_j0, then eps = eps + w_j * q_j over the further live roots (w_j != 0) in ascending j."""
    num, diag = np.atleast_2d(np.asarray(num, np.float64)), np.asarray(diag, np.float64)
    e, w = np.asarray(e, np.float64).reshape(-1), np.asarray(w, np.float64).reshape(-1)
    assert num.shape == (len(e), len(diag)) and w.shape == e.shape
    live = [j for j in range(len(w)) if w[j] != 0]
    assert live and np.all(np.isfinite(w)) and np.all(w >= 0)
    intruder, eps = np.zeros(len(diag), bool), None
    with np.errstate(all="ignore"):
        for j in live:
            den = diag - e[j]
            intruder |= ~(den > 0) | np.isnan(num[j])
            t = w[j] * ((num[j] * num[j]) / den)
            eps = t if eps is None else eps + t
        eps = np.where(intruder, np.inf, eps)
        eligible = (eps > 0) & (eps >= np.float64(eps_min))
    return eps, intruder, eligible


def select(keys, num, diag, e, w, k, eps_min=0.0, tie_rtol=1e-9):
    """sci_reference.select with the averaged importance: everything behind eps is the single-root rule, word for word."""
    keys = np.asarray(keys)
    eps, intruder, eligible = importance(num, diag, e, w, eps_min)
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


def loop(packed, keys0, n_roots, n_add, weights=None, eps_min=0.0, tie_rtol=1e-9):
    """-> dict(keys, eigs, vecs [n_roots, M], history=[dict(M, e0 [n_roots], e_pt2 [n_roots], n_external, n_intruders [n_roots],
    n_added, k, eps, tau, cut, next_root (the first eigenvalue left out, None at M = n_roots), min_den (the smallest |diag_a -
    e_j| over the rows and roots, None without rows))], stopped)."""
    ks, grow, n_iter = sci.schedule(n_add)
    w = equal_weights(n_roots) if weights is None else np.asarray(weights, np.float64)
    S = np.asarray(keys0, np.uint64).copy()
    assert len(S) >= n_roots
    Hss = sci.block(packed, S, S)
    history, stopped, lam, C = [], "schedule", None, None
    for t in range(n_iter):
        vals, vecs = np.linalg.eigh(Hss)
        lam, C = vals[:n_roots].copy(), vecs[:, :n_roots].T.copy()
        A = ref.connected_set(packed, S)
        Has = sci.block(packed, A, S)
        num, diag = (Has @ C.T).T, sci.diagonal(packed, A)
        e_pt2, n_intr = [], []
        for j in range(n_roots):
            eps_j, intr_j, _ = sci.importance(num[j], diag, lam[j])
            e_pt2.append(float(-np.sum(eps_j[~intr_j])))
            n_intr.append(int(intr_j.sum()))
        eps = importance(num, diag, lam, w)[0]
        rec = dict(M=len(S), e0=[float(x) for x in lam], e_pt2=e_pt2, n_external=len(A), n_intruders=n_intr, n_added=0, k=None, eps=eps,
                   tau=None, cut=None, next_root=float(vals[n_roots]) if len(vals) > n_roots else None,
                   min_den=float(np.min(np.abs(diag[None, :] - lam[:, None])[w != 0])) if len(A) else None)
        history.append(rec)
        if len(A) == 0:
            stopped = "connected set empty"
            break
        if t == n_iter - 1:
            break
        k = ks[t] if grow is None else int(math.ceil(grow * len(S)))
        sel, (n_sel, _), info = select(A, num, diag, lam, w, k, eps_min, tie_rtol)
        rec.update(k=k, tau=info["tau"], cut=info["cut"])
        if n_sel == 0:
            stopped = "nothing eligible"
            break
        rec["n_added"] = n_sel
        pick = info["mask"]
        Hss = np.block([[Hss, Has[pick].T], [Has[pick], sci.block(packed, sel, sel)]])
        S = np.concatenate([S, sel])
    return dict(keys=S, eigs=lam, vecs=C, history=history, stopped=stopped)


def gaps(history):
    """Per iteration the smallest gap between consecutive roots and from the last root to the first one left out."""
    out = []
    for h in history:
        lam = list(h["e0"]) + ([h["next_root"]] if h["next_root"] is not None else [])
        out.append(min(b - a for a, b in zip(lam, lam[1:])) if len(lam) > 1 else math.inf)
    return out


@lru_cache(maxsize=None)
def start(name, n_roots):
    """-> (packed, fci energy, the sector's n_roots determinants of lowest H_aa — stable argsort, ascending H_aa)."""
    packed, fci, _ = sci.start(name)
    keys = ref.sector_keys(packed.n_qubits, packed.n_alpha, packed.n_beta)
    return packed, fci, keys[np.argsort(sci.diagonal(packed, keys), kind="stable")[:n_roots]]


@lru_cache(maxsize=None)
def dense_run(name):
    """The dense loop of a schedule, equal weights: computed once, shared by the tests, never changed by them."""
    n_roots, n_add = SCHEDULES_ROOTS[name]
    packed, fci, k0 = start(name, n_roots)
    return loop(packed, k0, n_roots, n_add)


# fixture -> (roots, k of each growth step).  Left out on purpose: H2O with 4 roots at (4, 8, 16, 32) has an importance within
# 1e-6 of the cut at three steps; LiH with 2 roots from its two lowest determinants has at iteration 0 an external state with
# den ~ 0+ for root 1 (E_PT2 = -5e10); H2O with 2 roots at (2, 4, 8, 16, 32) has one with den = 0.0 exactly (the spin partner
# of root 1, tests/test_sci_roots.py) — with 3 roots both partners start inside and the same steps are clear.
SCHEDULES_ROOTS = {
    "LiH": (3, (3, 6, 12, 24)),
    "H2O": (3, (2, 4, 8, 16, 32)),
    "N2": (3, (4, 8, 16, 32, 64)),
}
