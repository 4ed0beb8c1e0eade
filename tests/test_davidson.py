"""The Davidson solver, the parts that need no GPU: the rule of include/naqs_hip.h: naqs_ham_eig_lowest as
tests/davidson_reference.py restates it, against numpy.linalg.eigh of the same dense block.

* every (fixture, M, seed) tests/test_davidson_gpu.py runs: the block is symmetric, the rule ends converged (or with a basis that
  spans the space), within 1e-9 Ha of the lowest eigenvalue, in at most 40 products — a condition on the cases, not a measurement
  (observed: at most 25);
* the rule's corners: M = 1, 2, 3; M below, at and above m_max; exact eigenvectors as starts; rows whose diagonal lies below theta;
  max_products; a start without a component outside the basis;
* why the correction is the positive-definite one: from the same start on LiH's full sector the rule finds the ground state and
  the textbook correction r / (theta - d) does not;
* the argument checks of ``lowest_eigenpair(solver=...)`` that come before any device call, ``eig_solver`` of the optimiser, and
  the ``-eig_solver`` switch of the command line, present and absent.
"""
import inspect
import os
import sys

import numpy as np
import pytest

import davidson_reference as dav
import pt2_reference as ref
from conftest import GOLDEN, PKG

LIH = os.path.join(GOLDEN, "ham_LiH.npz")
ALL_CASES = dav.CASES + tuple((name, None, None) for name in dav.WIDE)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_every_case_of_the_gpu_file(case):
    packed, keys, H, lam = dav.case(*case)
    M = len(keys)
    assert H.shape == (M, M) and len(np.unique(keys)) == M
    assert np.array_equal(H, H.T)
    got = dav.davidson(H, dav.random_start(M, case[2] or 0))
    print(f"{case}: M {M}, {got['products']} products, status {got['status']}, |theta - lambda_0| {abs(got['theta'] - lam):.2e}, rho {got['rho']:.2e}")
    assert got["status"] in (dav.CONVERGED, dav.SPANS)
    assert abs(got["theta"] - lam) <= 1e-9
    assert got["products"] <= 40
    assert abs(np.linalg.norm(got["vec"]) - 1.0) <= 1e-14


def test_the_unsymmetric_generators_are_why_their_symmetric_part_is_taken():
    import test_eloc_forms as F
    packed, keys, _ = F.crowded(64)
    H = dav.sci.block(packed, keys, keys)
    assert np.abs(H - H.T).max() > 1.0
    kept = dav.symmetric_part_of(packed)
    assert 0.25 * packed.K < kept.K < 0.75 * packed.K


def lih():
    packed, keys, H, w, v, fci = ref.molecule("LiH")
    return H, w, v


@pytest.mark.parametrize("M", [1, 2, 3])
def test_tiny_subspaces(M):
    H = lih()[0]
    S = ref.random_S(H.shape[0], M, 40 + M)
    B = H[np.ix_(S, S)]
    got = dav.davidson(B, dav.random_start(M, M))
    assert got["status"] in (dav.CONVERGED, dav.SPANS) and got["products"] <= M
    assert abs(got["theta"] - np.linalg.eigvalsh(B)[0]) <= 1e-12


@pytest.mark.parametrize("m_max", [2, 3, 8, 16, 32])
@pytest.mark.parametrize("M", [7, 8, 9, 40])
def test_basis_exhausts_and_restarts(M, m_max):
    """M below, at and above m_max: the basis spans the space (status 2, or converged on the way) or restarts and converges."""
    H = lih()[0]
    S = ref.random_S(H.shape[0], M, 3)
    B = H[np.ix_(S, S)]
    got = dav.davidson(B, dav.random_start(M, 1), m_max=m_max)
    assert got["status"] in (dav.CONVERGED, dav.SPANS) and abs(got["theta"] - np.linalg.eigvalsh(B)[0]) <= 1e-9
    if M <= m_max:
        assert got["products"] <= M                       # no restart can have happened
    else:
        assert got["status"] == dav.CONVERGED
        if m_max == 2:
            assert got["products"] > m_max                  # it did restart


def test_exact_eigenvectors_as_starts():
    """The ground vector: one product, converged.  An excited vector: a stationary point, returned as such — the solver finds the
    lowest state of what the start overlaps, it does not search the space the start is orthogonal to."""
    H, w, v = lih()
    got = dav.davidson(H, v[:, 0])
    assert (got["status"], got["products"]) == (dav.CONVERGED, 1) and abs(got["theta"] - w[0]) <= 1e-12
    got = dav.davidson(H, v[:, 5])
    assert (got["status"], got["products"]) == (dav.CONVERGED, 1) and abs(got["theta"] - w[5]) <= 1e-12 and w[5] - w[0] > 1e-3


def test_rows_below_theta_are_clamped():
    """At convergence theta <= min d (the variational principle), but the iteration starts at the random vector's Rayleigh
    quotient, in the middle of the spectrum: there rows with d_i < theta exist and meet the clamp.  The rule still converges to
    the lowest state; without the floor those rows' corrections would change sign."""
    H = lih()[0]
    S = ref.random_S(H.shape[0], 60, 8)
    B = H[np.ix_(S, S)]
    v0 = dav.random_start(60, 2)
    theta0 = v0 @ B @ v0 / (v0 @ v0)
    assert np.sum(np.diag(B) < theta0) >= 5
    got = dav.davidson(B, v0)
    assert got["status"] == dav.CONVERGED and abs(got["theta"] - np.linalg.eigvalsh(B)[0]) <= 1e-9 and got["products"] <= 40


def test_max_products_reached():
    H = lih()[0]
    got = dav.davidson(H, dav.random_start(H.shape[0], 0), max_products=3)
    assert (got["status"], got["products"]) == (dav.NOT_CONVERGED, 3)
    assert np.isfinite(got["theta"]) and np.all(np.isfinite(got["vec"])) and got["rho"] > 1e-6
    assert abs(got["theta"] - got["vec"] @ H @ got["vec"]) <= 1e-12            # the pair returned is a Ritz pair


def test_breakdown_is_reported():
    """A block-diagonal matrix and a start inside one block whose diagonal is constant: the correction is a multiple of the
    residual, and once the block is spanned nothing is left of it."""
    B = np.zeros((6, 6))
    B[:3, :3] = [[1.0, 0.1, 0.0], [0.1, 1.0, 0.1], [0.0, 0.1, 1.0]]
    B[3:, 3:] = np.diag([5.0, 6.0, 7.0])
    got = dav.davidson(B, np.array([1.0, 0.3, 0.2, 0, 0, 0]), tol=1e-300)
    assert got["status"] == dav.BREAKDOWN and got["products"] == 3 and abs(got["theta"] - np.linalg.eigvalsh(B[:3, :3])[0]) <= 1e-14


def test_why_the_correction_is_positive_definite():
    H, w, v = lih()
    start = dav.random_start(H.shape[0], 0)
    good = dav.davidson(H, start)
    assert good["status"] == dav.CONVERGED and abs(good["theta"] - w[0]) <= 1e-9
    bad = dav.davidson(H, start, textbook=True)
    print(f"LiH full sector: the rule {good['theta']:.10f} in {good['products']} products; r / (theta - d): {bad['theta']:.10f} "
          f"(status {bad['status']}, {bad['products']} products); lambda_0 {w[0]:.10f}, lambda_1 {w[1]:.10f}")
    assert not (bad["status"] == dav.CONVERGED and abs(bad["theta"] - w[0]) <= 1e-6)


# ---- arguments, the optimiser, the command line ---------------------------------------------------------------------------
def test_signatures_keep_their_defaults():
    sys.path.insert(0, PKG)
    from naqs_amd.hamiltonian import DevicePauliHamiltonian
    from naqs_amd.optimizer import PartialSamplingOptimizer
    p = inspect.signature(DevicePauliHamiltonian.lowest_eigenpair).parameters
    assert list(p)[:6] == ["self", "keys", "max_iter", "tol", "seed", "v0"]
    assert (p["solver"].default, p["m_max"].default, p["delta"].default) == ("lanczos", dav.M_MAX, dav.DELTA)
    assert inspect.signature(DevicePauliHamiltonian.selected_ci).parameters["solver"].default == "lanczos"
    assert inspect.signature(PartialSamplingOptimizer.__init__).parameters["eig_solver"].default == "lanczos"


class _Keys:
    shape = (4,)


def test_an_unknown_solver_is_refused_before_anything_runs():
    sys.path.insert(0, PKG)
    from naqs_amd.hamiltonian import DevicePauliHamiltonian
    from naqs_amd.optimizer import PartialSamplingOptimizer
    ham = object.__new__(DevicePauliHamiltonian)
    for bad in ("jacobi", None, "Davidson", 1):
        with pytest.raises(ValueError, match="solver"):
            DevicePauliHamiltonian.lowest_eigenpair(ham, _Keys(), solver=bad)
    with pytest.raises(ValueError, match="eig_solver"):
        PartialSamplingOptimizer(n_samples=10, eig_solver="jacobi")


def test_tile_mirror_reads_the_source():
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "naqs-for-quantum-chemistry_amd", "csrc", "naqs_eig.hip")).read()
    block = int(re.search(r"constexpr int EIG_BLOCK = (\d+);", src).group(1))
    pairs = int(re.search(r"constexpr int EIG_PAIRS = (\d+);", src).group(1))
    assert dav.T == block * pairs * 2
    assert int(re.search(r"constexpr int EIG_MMAX = (\d+);", src).group(1)) == 32


def _base():
    sys.path.insert(0, PKG)
    from experiments import _base
    return _base


def test_parser_accepts_eig_solver_and_lists_it_only_when_given(monkeypatch, capsys):
    _b = _base()
    p = _b.get_parser(n_hid=128)
    assert p.parse_args("-m molecules/LiH".split()).eig_solver is None
    assert p.parse_args("-m molecules/LiH -eig_solver davidson".split()).eig_solver == "davidson"
    with pytest.raises(SystemExit):
        p.parse_args("-m molecules/LiH -eig_solver jacobi".split())
    capsys.readouterr()
    seen = []
    monkeypatch.setattr(_b, "_run", lambda **kw: seen.append(kw) or [])
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-pt2"])
    assert "eig_solver" not in capsys.readouterr().out and "eig_solver" not in seen[-1]
    for choice in ("davidson", "lanczos"):
        _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-pt2", "-eig_solver", choice])
        assert f"\teig_solver : {choice}" in capsys.readouterr().out and seen[-1]["eig_solver"] == choice and seen[-1]["pt2"] is True


def test_switch_reaches_the_optimiser(tmp_path, monkeypatch):
    _b = _base()

    class Reached(Exception):
        pass

    def stop(*a, **kw):
        raise Reached(kw.get("eig_solver", "absent"))

    monkeypatch.setattr(_b, "_run_locked", stop)
    common = ["-m", LIH, "-o", str(tmp_path / "run"), "-s", "7"]
    with pytest.raises(Reached) as got:
        _b.run(n_hid=128, argv=common)
    assert got.value.args[0] == "absent"
    with pytest.raises(Reached) as got:
        _b.run(n_hid=128, argv=common + ["-eig_solver", "davidson"])
    assert got.value.args[0] == "davidson"
