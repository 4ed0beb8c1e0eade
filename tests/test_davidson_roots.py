"""The k-root Davidson solver, the parts that need no GPU: the rule of include/naqs_hip.h: naqs_ham_eig_lowest_k as
tests/davidson_roots_reference.py restates it, on every case tests/test_davidson_roots_gpu.py solves; the product counts that
file's caps come from; the reduction to naqs_ham_eig_lowest's rule at one root; argument checks, the optimiser's refusal on
the CPU and the command line's -roots.

Bounds: |theta_j - lambda_j| <= 1e-9 Ha against numpy.linalg.eigvalsh (the project's bound for a subspace energy);
X X^T - I <= 1e-12 (a basis orthonormal to O(m u) and an orthonormal S: about 32 * 32 * u = 2e-13).
"""
import inspect
import os
import sys

import numpy as np
import pytest

import davidson_reference as dav
import davidson_roots_reference as R
from conftest import GOLDEN, PKG

LIH = os.path.join(GOLDEN, "ham_LiH.npz")


# ---- the rule on the GPU file's cases -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES + (R.DEGENERATE,), ids=R.case_id)
def test_every_case_of_the_gpu_file(case):
    packed, keys, H, w = R.case(*case[:3])
    got = R.solved(case)
    k = min(case[3], len(keys))
    X = got["vecs"]
    err, orth = np.abs(got["theta"] - w[:k]).max(), np.abs(X @ X.T - np.eye(k)).max()
    print(f"{R.case_id(case)}: M {len(keys)}, status {got['status']}, {got['products']} products, |theta - lambda| {err:.1e}, "
          f"X X^T - I {orth:.1e}")
    assert got["theta"].shape == (k,) and X.shape == (k, len(keys))
    assert got["status"] in (R.CONVERGED, R.SPANS)
    assert err <= 1e-9 and orth <= 1e-12
    assert np.all(np.diff(got["theta"]) >= 0)


def test_product_counts_the_gpu_caps_come_from():
    """The GPU file allows products(case) + 2 k: these are the counts, pinned, and the gaps that keep the device on the rule's
    path (rounding may move a root's stopping iteration by one; with gaps >= 1e-3 Ha among the roots the paths do not fork)."""
    count = {R.case_id(c): R.products(c) for c in R.CASES}
    assert [count[f"LiH*-None-k{n}-m32"] for n in (2, 3, 4)] == [34, 57, 70]
    assert [count[f"H2O*-None-k{n}-m32"] for n in (2, 3, 4)] == [41, 67, 110]
    assert [count[f"N2-{M}-k4-m32"] for M in (2047, 2048, 2049, 4097)] == [78, 78, 78, 76]
    assert (count["N2-2049-k4-m16"], count["N2-2049-k4-m8"]) == (101, 215)
    assert [count[f"{n}-None-k3-m32"] for n in dav.WIDE] == [33, 29, 32, 34]
    for c in R.CASES:
        k = min(c[3], len(R.case(*c[:3])[1]))
        assert R.cap(c) == count[R.case_id(c)] + 2 * k and count[R.case_id(c)] <= R.cap(c) <= 400
    # a restart every iteration at m_max = 2 k, none needed below it at 32 for the small cases
    assert count["N2-2049-k4-m8"] > count["N2-2049-k4-m16"] > count["N2-2049-k4-m32"]


@pytest.mark.parametrize("case", dav.CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_one_root_is_the_single_root_rule(case):
    packed, keys, H, lam = dav.case(*case)
    v0 = dav.random_start(len(keys), case[2])
    one = dav.davidson(H, v0, tol=R.TOL)
    blk = R.davidson_k(H, v0[None], tol=R.TOL, m_max=dav.M_MAX)
    assert (blk["products"], blk["status"]) == (one["products"], one["status"])
    assert abs(blk["theta"][0] - one["theta"]) <= 1e-13 and abs(abs(blk["vecs"][0] @ one["vec"]) - 1.0) <= 1e-10


def test_statuses_and_refused_starts():
    packed, keys, H, w = R.case("LiH", 17, 28)
    v0 = R.starts(17, 28, 2)
    few = R.davidson_k(H, v0, max_products=4)
    assert few["status"] == R.NOT_CONVERGED and 4 <= few["products"] < 4 + 2
    spans = R.davidson_k(H[:3, :3], R.starts(3, 1, 4))
    assert spans["status"] in (R.CONVERGED, R.SPANS) and spans["products"] == 3 and len(spans["theta"]) == 3
    for bad in (np.array([v0[0], v0[0]]), np.array([v0[0], 0 * v0[0]]), np.array([v0[0], np.full(17, np.nan)])):
        with pytest.raises(ValueError):
            R.davidson_k(H, bad)
    for kw in (dict(m_max=3), dict(m_max=33)):
        with pytest.raises(ValueError):
            R.davidson_k(H, v0, **kw)


# ---- arguments, the optimiser, the command line ---------------------------------------------------------------------------
class _Keys:
    shape = (40,)
    is_cuda = False


def test_arguments_are_checked_before_anything_runs():
    sys.path.insert(0, PKG)
    from naqs_amd.hamiltonian import DevicePauliHamiltonian
    p = inspect.signature(DevicePauliHamiltonian.lowest_eigenpairs).parameters
    assert list(p) == ["self", "keys", "k", "max_iter", "tol", "seed", "v0", "m_max", "delta"]
    assert [p[n].default for n in ("max_iter", "tol", "seed", "v0", "m_max", "delta")] == [400, 1e-10, 0, None, R.M_MAX, R.DELTA]
    ham = object.__new__(DevicePauliHamiltonian)
    for bad in (dict(k=0), dict(k=9), dict(k=2, m_max=3), dict(k=4, m_max=7), dict(k=1, m_max=33), dict(k=2, tol=0.0),
                dict(k=2, tol=float("nan")), dict(k=2, delta=0.0), dict(k=2, delta=float("inf")), dict(k=2, max_iter=0)):
        with pytest.raises(ValueError, match="k must|m_max|max_iter"):
            DevicePauliHamiltonian.lowest_eigenpairs(ham, _Keys(), **bad)
    with pytest.raises(ValueError, match="device tensor"):
        DevicePauliHamiltonian.lowest_eigenpairs(ham, _Keys(), 2)
    # the single-root entry keeps its defaults
    q = inspect.signature(DevicePauliHamiltonian.lowest_eigenpair).parameters
    assert (q["solver"].default, q["m_max"].default) == ("lanczos", dav.M_MAX)


def test_the_optimiser_refuses_on_the_cpu():
    sys.path.insert(0, PKG)
    import torch
    from naqs_amd.optimizer import PartialSamplingOptimizer
    p = inspect.signature(PartialSamplingOptimizer.solve_H_roots).parameters
    assert [(n, p[n].default) for n in list(p)[1:]] == [("n_samps", None), ("n_roots", 2), ("pt2", False)]
    opt = object.__new__(PartialSamplingOptimizer)
    opt.device = torch.device("cpu")
    with pytest.raises(NotImplementedError, match="HIP"):
        opt.solve_H_roots(n_samps=10)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="n_roots"):
            opt.solve_H_roots(n_samps=10, n_roots=bad)


def _base():
    sys.path.insert(0, PKG)
    from experiments import _base
    return _base


def test_parser_accepts_roots_and_lists_it_only_when_given(monkeypatch, capsys):
    _b = _base()
    p = _b.get_parser(n_hid=128)
    assert p.parse_args("-m molecules/LiH".split()).roots is None
    assert p.parse_args("-m molecules/LiH -roots 3".split()).roots == 3
    with pytest.raises(SystemExit):
        p.parse_args("-m molecules/LiH -roots two".split())
    capsys.readouterr()
    seen = []
    monkeypatch.setattr(_b, "_run", lambda **kw: seen.append(kw) or [])
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-pt2"])
    assert "roots" not in capsys.readouterr().out and "roots" not in seen[-1]
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-pt2", "-roots", "4"])
    assert "\troots : 4" in capsys.readouterr().out and seen[-1]["roots"] == 4 and seen[-1]["pt2"] is True
    for bad in ("0", "9", "-1"):
        with pytest.raises(ValueError, match="-roots"):
            _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-roots", bad])
    assert len(seen) == 2


def test_roots_lines_of_the_summary():
    _b = _base()
    roots = dict(eigs=[-7.5, -7.25, -7.0], n_unq=40)
    lines = _b._roots_lines(roots)
    assert lines == ["sampled-subspace root 0 (40 states) : -7.50000000 , gap to root 0 0.0000 mHa",
                     "sampled-subspace root 1 (40 states) : -7.25000000 , gap to root 0 250.0000 mHa",
                     "sampled-subspace root 2 (40 states) : -7.00000000 , gap to root 0 500.0000 mHa"]
    with_pt2 = _b._roots_lines(dict(roots, e_pt2=[-0.001, -0.002, -0.003]))
    assert [ln[len(l0):] for ln, l0 in zip(with_pt2, lines)] == [" , E + E_PT2 -7.50100000", " , E + E_PT2 -7.25200000", " , E + E_PT2 -7.00300000"]


def test_the_library_declares_the_entry_points_and_their_limits():
    import re
    from conftest import ROOT
    from naqs_amd import _lib
    assert {"naqs_ham_block_product", "naqs_ham_eig_lowest_k"} <= set(_lib.SIGNATURES)
    src = open(os.path.join(ROOT, "naqs-for-quantum-chemistry_amd", "csrc", "naqs_eig.hip")).read()
    assert int(re.search(r"constexpr int KR = (\d+);", src).group(1)) == 8
    header = open(os.path.join(ROOT, "include", "naqs_hip.h")).read()
    assert "int naqs_ham_eig_lowest_k(" in header and "int naqs_ham_block_product(" in header
