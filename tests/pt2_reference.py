"""The dense float64 reference of the second-order Epstein-Nesbet correction (a plain helper module, like sr_reference.py).

For a subspace S of a particle-number sector, a vector c on S and an energy e0:

    r_a   = sum_{j in S} H_aj c_j              a not in S
    E_PT2 = sum_{a: e0 - H_aa < 0} r_a^2 / (e0 - H_aa)

over ALL a outside S — a state that no Hamiltonian term connects to S has r_a = 0 exactly, so the sum over the connected set
(what include/naqs_hip.h: naqs_ham_pt2 is given) is the same number.  A state with e0 - H_aa >= 0 (an "intruder") is left out
and counted.

* ``sector_keys``   the keys of a sector, ascending; even qubits alpha, odd qubits beta (the packing's convention);
* ``dense_H``       H[i, key_i ^ xy_k] += coeff_k (-1)^popcount(key_i & yz_k), the definition every kernel restates;
* ``top_S``         the M states of largest |coefficient| in the exact ground state;
* ``random_S``      M states drawn without replacement;
* ``ground``        lowest eigenpair of H[S, S];
* ``pt2``           the six quantities of DevicePauliHamiltonian.pt2_correction, plus r and the diagonal per external state;
* ``abs_bound``     sum over a row's partners in S of (sum of the group's |coeff|) |c_j|: the magnitude its error is held against
                    (``dense_abs``: the same for every row at once, as a matrix; ``diag_bound``: the diagonal group's);
* ``connected_set`` the keys ``naqs_ham_connected`` returns for a table, from the definition;
* ``molecule``      a committed fixture's packed terms, sector keys, dense H, spectrum and FCI energy, built once.
"""
import os
from functools import lru_cache

import numpy as np

from conftest import GOLDEN


def sector_keys(N, na, nb):
    """Ascending keys of N qubits with na set bits on the even positions and nb on the odd ones."""
    k = np.arange(1 << N, dtype=np.uint64)
    n_even = sum(((k >> np.uint64(q)) & np.uint64(1)).astype(np.int64) for q in range(0, N, 2))
    n_odd = sum(((k >> np.uint64(q)) & np.uint64(1)).astype(np.int64) for q in range(1, N, 2))
    return k[(n_even == na) & (n_odd == nb)]


def _parity(x):
    x = x.copy()
    for s in (32, 16, 8, 4, 2, 1):
        x ^= x >> np.uint64(s)
    return (x & np.uint64(1)).astype(np.int64)


def dense_H(packed, keys):
    """H over `keys` (ascending): rows i, columns the position of key_i ^ xy_k where that key is in `keys`."""
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    H = np.zeros((n, n))
    rows = np.arange(n)
    for xy, yz, cf in zip(packed.xy, packed.yz, packed.coeff):
        j = keys ^ np.uint64(xy)
        pos = np.minimum(np.searchsorted(keys, j), n - 1)
        ok = keys[pos] == j
        sign = 1.0 - 2.0 * _parity(keys & np.uint64(yz))
        np.add.at(H, (rows[ok], pos[ok]), cf * sign[ok])
    return H


@lru_cache(maxsize=None)
def molecule(name):
    """-> (packed, sector keys, dense H, eigenvalues, eigenvectors, fci_energy) of a committed fixture."""
    from naqs_amd import packing
    path = os.path.join(GOLDEN, f"ham_{name}.npz")
    packed = packing.load_packed(path)
    keys = sector_keys(packed.n_qubits, packed.n_alpha, packed.n_beta)
    H = dense_H(packed, keys)
    w, v = np.linalg.eigh(H)
    with np.load(path) as z:
        fci = float(z["fci_energy"])
    return packed, keys, H, w, v, fci


def top_S(H, M):
    w, v = np.linalg.eigh(H)
    return np.sort(np.argsort(-np.abs(v[:, 0]), kind="stable")[:M])


def random_S(n, M, seed):
    return np.random.RandomState(seed).permutation(n)[:M]


def ground(H, S):
    w, v = np.linalg.eigh(H[np.ix_(S, S)])
    c = v[:, 0]
    return float(w[0]), c * (1.0 if c[np.argmax(np.abs(c))] > 0 else -1.0)


def pt2(H, S, c, e0):
    """-> dict(e0, e_pt2, n_external, n_intruders, residual2, intruder_residual2, ext (indices outside S), r, diag)."""
    S = np.asarray(S)
    ext = np.setdiff1d(np.arange(H.shape[0]), S)
    r = H[np.ix_(ext, S)] @ np.asarray(c, np.float64)
    diag = H[ext, ext]
    den = e0 - diag
    ok = den < 0
    return dict(e0=float(e0), e_pt2=float(np.sum(r[ok] ** 2 / den[ok])), n_external=len(ext), n_intruders=int(np.sum(~ok)),
                residual2=float(np.sum(r[ok] ** 2)), intruder_residual2=float(np.sum(r[~ok] ** 2)), ext=ext, r=r, diag=diag)


def group_abs(packed):
    """flip mask -> sum of |coeff| of its terms."""
    out = {}
    for xy, cf in zip(packed.xy, packed.coeff):
        out[int(xy)] = out.get(int(xy), 0.0) + abs(float(cf))
    return out


def abs_bound(packed, keys_S, c, a, groups=None):
    """sum over the partners j = a ^ xy_g (xy_g != 0) that S holds of (sum_{t in g} |coeff_t|) |c_j|."""
    groups = group_abs(packed) if groups is None else groups
    at = {int(k): i for i, k in enumerate(np.asarray(keys_S, np.uint64))}
    total = 0.0
    for xy, mag in groups.items():
        if xy and (int(a) ^ xy) in at:
            total += mag * abs(float(c[at[int(a) ^ xy]]))
    return total


def dense_abs(packed, keys):
    """dense_H with |coeff| and no sign: entry (a, j) is the sum of |coeff| over the group a ^ j.  ``dense_abs[ext][:, S] @ |c|``
    is ``abs_bound`` of every external row at once."""
    from naqs_amd.packing import PackedHamiltonian
    return dense_H(PackedHamiltonian(packed.n_qubits, packed.n_alpha, packed.n_beta, packed.xy, np.zeros_like(packed.yz),
                                     np.abs(packed.coeff)), keys)


def diag_bound(packed):
    return group_abs(packed).get(0, 0.0)


def connected_set(packed, keys_S):
    """The keys naqs_ham_connected returns for the whole table: j = key ^ xy_g (xy_g != 0) in the sector and not in S, ascending."""
    keys_S = np.asarray(keys_S, np.uint64)
    masks = np.unique(packed.xy)
    masks = masks[masks != 0]
    j = np.unique((keys_S[:, None] ^ masks[None, :]).ravel())
    if packed.n_alpha >= 0:
        N = packed.n_qubits
        n_even = sum(((j >> np.uint64(q)) & np.uint64(1)).astype(np.int64) for q in range(0, N, 2))
        n_odd = sum(((j >> np.uint64(q)) & np.uint64(1)).astype(np.int64) for q in range(1, N, 2))
        j = j[(n_even == packed.n_alpha) & (n_odd == packed.n_beta)]
    return np.setdiff1d(j, keys_S)
