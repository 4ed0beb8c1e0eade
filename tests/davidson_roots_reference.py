"""The reference of the k-root Davidson solver (a plain helper module, like davidson_reference.py): the rule of
include/naqs_hip.h: naqs_ham_eig_lowest_k restated in NumPy on a dense float64 block.

* ``davidson_k``  the rule: -> dict(theta [k], vecs [k, M], rho [k], products, status); a rank-deficient, zero or non-finite
                  start raises ValueError (the library's NAQS_ERR_INVALID);
* ``starts``      the k starts of a case: row j is ``davidson_reference.random_start(M, seed + 100 j)``;
* ``CASES``       every (fixture, M, seed, n_roots, m_max) tests/test_davidson_roots_gpu.py solves; tests/test_davidson_roots.py
                  checks the rule on each and pins the product counts the GPU file's caps are derived from;
* ``products``    the rule's product count of a case (cached: computed once per session, shared by both test files).
"""
from functools import lru_cache

import numpy as np

import davidson_reference as dav
import pt2_reference as ref

M_MAX = 32
DELTA = dav.DELTA
TOL = 1e-10
CONVERGED, NOT_CONVERGED, SPANS, BREAKDOWN = dav.CONVERGED, dav.NOT_CONVERGED, dav.SPANS, dav.BREAKDOWN


def _twice(V, t):
    for _ in range(2):
        if V:
            Vm = np.array(V)
            t = t - Vm.T @ (Vm @ t)
    return t


def davidson_k(H, v0, tol=TOL, max_products=400, m_max=M_MAX, delta=DELTA):
    H = np.asarray(H, np.float64)
    M = H.shape[0]
    v0 = np.atleast_2d(np.asarray(v0, np.float64))
    n_roots = v0.shape[0]
    if not (1 <= n_roots <= 8 and 2 * n_roots <= m_max <= 32):
        raise ValueError("n_roots in 1..8, m_max in 2 n_roots..32")
    k = min(n_roots, M)
    d = np.diag(H).copy()
    V = []
    for j in range(k):
        before = np.linalg.norm(v0[j])
        with np.errstate(all="ignore"):
            t = _twice(V, v0[j].copy())
            nt = np.linalg.norm(t)
        if not np.isfinite(nt) or not nt > 1e-14 * before:
            raise ValueError(f"start row {j} is zero, non-finite or depends on the rows before it")
        V.append(t / nt)
    W = [H @ v for v in V]
    products = k
    while True:
        m = len(V)
        Vm, Wm = np.array(V), np.array(W)
        G = np.triu(Vm @ Wm.T)
        G = G + np.triu(G, 1).T
        w, S = np.linalg.eigh(G)
        theta = w[:k].copy()
        S = (S[:, :k] / np.linalg.norm(S[:, :k], axis=0)).T
        X, Y = S @ Vm, S @ Wm
        R = Y - theta[:, None] * X
        rho = np.linalg.norm(R, axis=1)
        open_ = [j for j in range(k) if not rho[j] < tol * max(1.0, abs(theta[j]))]
        if not open_:
            status = CONVERGED
            break
        if m == M:
            status = SPANS
            break
        if products >= max_products:
            status = NOT_CONVERGED
            break
        if m + len(open_) > m_max:
            nx = np.linalg.norm(X, axis=1)
            V, W = [X[j] / nx[j] for j in range(k)], [Y[j] / nx[j] for j in range(k)]
        accepted = 0
        for j in open_:
            if len(V) >= M:
                break
            with np.errstate(all="ignore"):
                t = -R[j] / np.maximum(d - theta[j], delta)
                before = np.linalg.norm(t)
                t = _twice(V, t)
                nt = np.linalg.norm(t)
            if not np.isfinite(nt) or nt <= 1e-14 * before:
                continue
            V.append(t / nt)
            W.append(H @ (t / nt))
            products += 1
            accepted += 1
        if accepted == 0:
            status = BREAKDOWN
            break
    return dict(theta=theta, vecs=X / np.linalg.norm(X, axis=1)[:, None], rho=rho, products=products, status=status)


def starts(M, seed, n_roots):
    return np.array([dav.random_start(M, seed + 100 * j) for j in range(n_roots)])


@lru_cache(maxsize=None)
def case(name, M=None, seed=None):
    """-> (packed, keys, dense block, eigenvalues ascending) of a subset case, a wide-key case or a full sector ("LiH*", "H2O*")."""
    if name.endswith("*"):
        packed, keys, H, w, v, fci = ref.molecule(name[:-1])
        return packed, np.asarray(keys, np.uint64), H, np.asarray(w)
    packed, keys, H, _ = dav.case(name, M, seed)
    return packed, keys, H, np.linalg.eigvalsh(H)


# (fixture, M, seed of the subset and of the starts, n_roots, m_max)
SIZES = tuple(("LiH", M, 11 + M, n, M_MAX) for M in (1, 2, 3, 15, 16, 17, 63, 64, 65) for n in (2, 4)) + \
    tuple(("N2", M, 5, 4, M_MAX) for M in (dav.T - 1, dav.T, dav.T + 1, 2 * dav.T + 1))
WIDE = tuple((name, None, 0, 3, M_MAX) for name in dav.WIDE)
SECTORS = tuple((mol + "*", None, 0, n, M_MAX) for mol in ("LiH", "H2O") for n in (2, 3, 4))
RESTARTS = tuple(("N2", dav.T + 1, 5, 4, m_max) for m_max in (8, 16))
CASES = SIZES + WIDE + SECTORS + RESTARTS
DEGENERATE = ("LiH*", None, 0, 8, M_MAX)           # the eight lowest hold a degenerate pair: no product count is taken from it


def case_id(c):
    return f"{c[0]}-{c[1]}-k{c[3]}-m{c[4]}"


@lru_cache(maxsize=None)
def solved(c):
    name, M, seed, n_roots, m_max = c
    packed, keys, H, w = case(name, M, seed)
    return davidson_k(H, starts(len(keys), seed, n_roots), tol=TOL, m_max=m_max)


def products(c):
    return solved(c)["products"]


def cap(c):
    """What the device may spend on a case: the rule's count, and one iteration's rounding slack per root (a root whose
    residual sits at the tolerance may close an iteration later on the device, or earlier, and costs a product each time)."""
    return products(c) + 2 * len(solved(c)["theta"])
