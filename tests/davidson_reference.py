"""The reference of the Davidson solver (a plain helper module, like sci_reference.py): the rule of
include/naqs_hip.h: naqs_ham_eig_lowest restated in NumPy on a dense float64 block.

* ``davidson``     the rule: -> dict(theta, vec, rho, products, status); ``textbook=True`` swaps the correction for the textbook
                   r / (theta - d) and changes nothing else (tests/test_davidson.py pins why the rule does not use it);
* ``random_start`` a seeded start on the host (the device tests hand the same vector to both sides);
* ``subset_block`` the dense block of a random subset of a fixture's sector, built once per (fixture, M, seed);
* ``symmetric_part_of`` a packed Hamiltonian without the terms whose popcount(xy & yz) is odd — what is left is symmetric;
* ``CASES``        every (fixture, M, seed) tests/test_davidson_gpu.py runs; tests/test_davidson.py checks the rule on each.
"""
from functools import lru_cache

import numpy as np

import pt2_reference as ref
import sci_reference as sci

T = 2048                          # elements a workgroup takes (naqs_eig.hip: EIG_TILE)
M_MAX = 16
DELTA = 1e-2

CONVERGED, NOT_CONVERGED, SPANS, BREAKDOWN = 0, 1, 2, 3


def davidson(H, v0, tol=1e-10, max_products=400, m_max=M_MAX, delta=DELTA, textbook=False):
    H = np.asarray(H, np.float64)
    M = H.shape[0]
    d = np.diag(H).copy()
    v = np.asarray(v0, np.float64) / np.linalg.norm(v0)
    V, W = [v], [H @ v]
    products = 1
    while True:
        m = len(V)
        Vm, Wm = np.array(V), np.array(W)
        G = np.triu(Vm @ Wm.T)
        G = G + np.triu(G, 1).T
        w, S = np.linalg.eigh(G)
        theta, s = float(w[0]), S[:, 0] / np.linalg.norm(S[:, 0])
        x, y = s @ Vm, s @ Wm
        r = y - theta * x
        rho = float(np.linalg.norm(r))
        if rho < tol * max(1.0, abs(theta)):
            status = CONVERGED
            break
        if m == M:
            status = SPANS
            break
        if products == max_products:
            status = NOT_CONVERGED
            break
        with np.errstate(all="ignore"):
            t = r / (theta - d) if textbook else -r / np.maximum(d - theta, delta)
        if m == m_max:
            nx = np.linalg.norm(x)
            V, W = [x / nx], [y / nx]
        before = np.linalg.norm(t)
        for _ in range(2):
            Vm = np.array(V)
            t = t - Vm.T @ (Vm @ t)
        nt = np.linalg.norm(t)
        if not np.isfinite(nt) or nt <= 1e-14 * before:
            status = BREAKDOWN
            break
        v = t / nt
        V.append(v)
        W.append(H @ v)
        products += 1
    return dict(theta=theta, vec=x / np.linalg.norm(x), rho=rho, products=products, status=status)


def random_start(M, seed=0):
    return np.random.RandomState(1000 + seed).normal(size=M)


@lru_cache(maxsize=None)
def sector(mol):
    """-> (packed, sector keys ascending) of a committed fixture, without its dense matrix (N2's sector has 14 400 states)."""
    import os
    from conftest import GOLDEN
    from naqs_amd import packing
    packed = packing.load_packed(os.path.join(GOLDEN, f"ham_{mol}.npz"))
    return packed, ref.sector_keys(packed.n_qubits, packed.n_alpha, packed.n_beta)


@lru_cache(maxsize=None)
def subset_block(mol, M, seed):
    """-> (packed, keys [M] in random order, dense block, lowest eigenvalue)."""
    packed, keys = sector(mol)
    S = keys[ref.random_S(len(keys), M, seed)]
    H = sci.block(packed, S, S)
    return packed, S, H, float(np.linalg.eigvalsh(H)[0])


def symmetric_part_of(packed):
    from naqs_amd.packing import PackedHamiltonian
    xy, yz = np.asarray(packed.xy, np.uint64), np.asarray(packed.yz, np.uint64)
    keep = sci._parity(xy & yz) == 0
    return PackedHamiltonian(packed.n_qubits, packed.n_alpha, packed.n_beta, xy[keep], yz[keep], np.asarray(packed.coeff)[keep])


WIDE = ("heavy64", "crowded64", "heavy32", "crowded32")


@lru_cache(maxsize=None)
def wide_case(name):
    """The 40-qubit (64-bit keys) and 32-qubit generators of tests/test_eloc_forms.py — the instance matrix's 1 499 keys and the
    crowded table's 512 — with the symmetric part of their Hamiltonians.  -> (packed, keys, dense block, lowest eigenvalue)."""
    import test_eloc_forms as F
    kb = int(name[-2:])
    N, na, nb = {32: (32, 8, 8), 64: (40, 6, 6)}[kb]
    if name.startswith("crowded"):
        packed, keys, _ = F.crowded(kb)
    else:
        keys = F.matrix_keys(N, na, nb)
        packed = F.ham_with_heavy_groups(keys, F.MATRIX_MASKS, 5, na, nb, N)
    packed = symmetric_part_of(packed)
    keys = np.asarray(keys, np.uint64)
    H = sci.block(packed, keys, keys)
    return packed, keys, H, float(np.linalg.eigvalsh(H)[0])


def case(name, M=None, seed=None):
    return wide_case(name) if name in WIDE else subset_block(name, M, seed)


# (fixture, M, seed of the subset); the start is random_start(M, seed)
CASES = tuple(("LiH", M, 11 + M) for M in (1, 2, 3, 15, 16, 17, 63, 64, 65)) + \
    tuple(("N2", M, 5) for M in (T - 1, T, T + 1, 2 * T + 1))
