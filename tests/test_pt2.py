"""Epstein-Nesbet second-order correction of the sampled-subspace energy, the parts that need no GPU: the dense float64
reference of tests/pt2_reference.py and what it says about the gain on the committed LiH and H2O fixtures, the C-ABI surface
of ``naqs_ham_pt2``, the ``-pt2`` switch from the command line to the optimiser and into summary.txt, and the refusal of
``solve_H_pt2`` without a device.  tests/test_pt2_gpu.py holds the kernel to the same reference."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

import pt2_reference as ref
from conftest import GOLDEN, PKG, ROOT
from naqs_amd import _lib

torch = pytest.importorskip("torch")
LIH = os.path.join(GOLDEN, "ham_LiH.npz")
SIZES = {"LiH": 225, "H2O": 441}
TOP_M = (1, 2, 3, 17, 63, 64, 65, 129, 200)


def subspace(mol, S):
    packed, keys, H, w, v, fci = ref.molecule(mol)
    e0, c = ref.ground(H, S)
    return e0, c, ref.pt2(H, S, c, e0), fci


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol", ["LiH", "H2O"])
def test_dense_hamiltonian_is_the_fixtures(mol):
    packed, keys, H, w, v, fci = ref.molecule(mol)
    assert len(keys) == SIZES[mol] and np.all(np.diff(keys.astype(np.int64)) > 0)
    even = sum(1 << q for q in range(0, packed.n_qubits, 2))
    assert all(bin(int(k) & even).count("1") == packed.n_alpha and bin(int(k) & ~even).count("1") == packed.n_beta for k in keys)
    assert np.array_equal(H, H.T)
    print(f"{mol}: lowest eigenvalue - fci_energy = {w[0] - fci:.3e}")
    assert abs(w[0] - fci) < 1e-13 * max(1.0, abs(fci))


@pytest.mark.parametrize("mol,M,gain", [("LiH", 17, 1e-6), ("LiH", 3, None), ("H2O", 17, None), ("H2O", 63, 1e-7)])
def test_the_correction_recovers_the_energy_outside_the_subspace(mol, M, gain):
    """E_S - FCI, E_PT2 and what is left, recomputed: the corrected energy is two to three orders of magnitude closer."""
    packed, keys, H, w, v, fci = ref.molecule(mol)
    e0, c, res, _ = subspace(mol, ref.top_S(H, M))
    left = e0 + res["e_pt2"] - fci
    print(f"{mol} M={M}: E_S - FCI {e0 - fci:.3e}, E_PT2 {res['e_pt2']:.4e}, E_S + E_PT2 - FCI {left:+.2e}")
    assert e0 - fci > 0 and res["e_pt2"] < 0 and res["n_intruders"] == 0 and res["n_external"] == len(keys) - M
    assert abs(left) < 1e-2 * (e0 - fci)
    if gain is not None:
        assert abs(left) < gain


@pytest.mark.parametrize("mol", ["LiH", "H2O"])
def test_reference_invariants(mol):
    packed, keys, H, w, v, fci = ref.molecule(mol)
    n = len(keys)
    # the whole sector: nothing outside, nothing to correct
    e0, c, res, _ = subspace(mol, np.arange(n))
    assert res["n_external"] == 0 and res["e_pt2"] == 0.0 and res["residual2"] == 0.0 and abs(e0 - fci) < 1e-12
    assert len(ref.connected_set(packed, keys)) == 0
    S = ref.top_S(H, 17)
    e0, c, res, _ = subspace(mol, S)
    # r is the residual of (c, 0) in the whole sector: H (c, 0) - e0 (c, 0) vanishes on S and is r outside
    full = np.zeros(n)
    full[S] = c
    resid = H @ full - e0 * full
    assert np.max(np.abs(resid[S])) < 1e-12 and np.allclose(resid[res["ext"]], res["r"], rtol=0, atol=1e-15)
    assert abs(res["residual2"] + res["intruder_residual2"] - float(resid @ resid)) < 1e-12
    # a state no term connects to S has r = 0 exactly, and the connected set is the rest
    conn = ref.connected_set(packed, keys[S])
    off = np.setdiff1d(keys[res["ext"]], conn)
    assert len(conn) + len(off) == n - 17 and np.all(res["r"][np.isin(keys[res["ext"]], off)] == 0.0)
    # abs_bound bounds |r_a| term by term
    groups = ref.group_abs(packed)
    for a, r in zip(keys[res["ext"]][:40], res["r"][:40]):
        assert abs(r) <= ref.abs_bound(packed, keys[S], c, a, groups) * (1 + 1e-12)
    assert np.all(np.abs(res["diag"]) <= ref.diag_bound(packed))
    bounds = ref.dense_abs(packed, keys)[np.ix_(res["ext"][:40], S)] @ np.abs(c)
    assert np.allclose(bounds, [ref.abs_bound(packed, keys[S], c, a, groups) for a in keys[res["ext"]][:40]], rtol=1e-13, atol=0)
    # the sign of c does not enter, its scale enters squared
    twice = ref.pt2(H, S, -2.0 * c, e0)
    assert twice["e_pt2"] == pytest.approx(4.0 * res["e_pt2"], rel=1e-14)


@pytest.mark.parametrize("mol", ["LiH", "H2O"])
def test_no_intruder_among_the_largest_coefficients(mol):
    packed, keys, H, w, v, fci = ref.molecule(mol)
    worst = -np.inf
    for M in TOP_M + (len(keys) - 1,):
        e0, c, res, _ = subspace(mol, ref.top_S(H, M))
        assert res["n_intruders"] == 0 and res["e_pt2"] <= 0.0, M
        worst = max(worst, float(np.max(e0 - res["diag"])))
    print(f"{mol}: largest denominator over the subspaces {worst:.3f}")
    assert worst < -0.1


@pytest.mark.parametrize("mol", ["LiH", "H2O"])
def test_random_subspaces_have_intruders(mol):
    """A subspace that misses the dominant determinants has external states below its energy: the branch the kernel keeps out
    of the sum.  (Counts here: LiH 25, 3, 1 and H2O 16, 5, 5 at M = 17, 65, 130.)"""
    packed, keys, H, w, v, fci = ref.molecule(mol)
    for M in (17, 65, 130):
        S = ref.random_S(len(keys), M, 7)
        e0, c, res, _ = subspace(mol, S)
        print(f"{mol} random M={M}: {res['n_intruders']} intruders, residual^2 {res['intruder_residual2']:.3e} of {res['residual2']:.3e}")
        assert res["n_intruders"] > 0
        den = e0 - res["diag"]
        assert res["e_pt2"] == pytest.approx(float(np.sum((res["r"] ** 2 / den)[den < 0])), rel=1e-14) and res["e_pt2"] <= 0.0


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "naqs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint naqs_ham_pt2\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 11
    for arg in ("const double *c_dev", "double e0", "const uint64_t *ext_keys_dev", "double *num_dev", "double *diag_dev", "double *out4_dev"):
        assert arg in m.group(1)
    res, args = _lib.SIGNATURES["naqs_ham_pt2"]
    assert res is ctypes.c_int and len(args) == 11 and args[4] is ctypes.c_double
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "naqs_ham_pt2")
    assert int(re.search(r"#define NAQS_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 9      # an addition
    assert _lib.load_library().naqs_ham_pt2(None, 1, None, None, 0.0, 0, None, None, None, None, None) == -1


# ---- the optimiser and the command line ----------------------------------------------------------------------------------
def test_solve_h_pt2_needs_a_device():
    from naqs_amd.optimizer import OptimizerBase, PartialSamplingOptimizer
    assert issubclass(PartialSamplingOptimizer, OptimizerBase)
    opt = object.__new__(PartialSamplingOptimizer)
    opt.device = torch.device("cpu")
    with pytest.raises(NotImplementedError, match="solve_H_pt2"):
        opt.solve_H_pt2(n_samps=10)


def _base():
    sys.path.insert(0, PKG)
    from experiments import _base
    return _base


class Reached(Exception):
    pass


class FakeOptimizer:
    """Stands where PartialSamplingOptimizer does in experiments._base: trains nothing, says which solve was asked for."""
    n_samples = 1234
    calls = []

    def __init__(self, **kw):
        self.save_loc = kw["save_loc"]

    def pre_flatten(self, *a, **kw):
        pass

    def save(self):
        pass

    def run(self, **kw):
        pass

    def solve_H(self, n_samps=None, ret_n_samps=True):
        FakeOptimizer.calls.append(("solve_H", n_samps))
        return -7.5, 0.9, 40

    def solve_H_pt2(self, n_samps=None):
        FakeOptimizer.calls.append(("solve_H_pt2", n_samps))
        return dict(eig=-7.5, vec0=0.9, n_unq=40, e_pt2=-1e-3, n_external=150, n_intruders=0)


COMMON = ["-m", LIH, "-single_phase", "-n_hid", "16", "-n_hid_phase", "32", "-n_train", "2", "-s", "7", "-lr", "0.001"]


def test_parser_accepts_pt2_and_lists_it_only_when_given(monkeypatch, capsys):
    _b = _base()
    p = _b.get_parser(n_hid=128)
    assert p.parse_args("-m molecules/LiH".split()).pt2 is False and p.parse_args("-m molecules/LiH -pt2".split()).pt2 is True
    seen = []
    monkeypatch.setattr(_b, "_run", lambda **kw: seen.append(kw) or [])
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7"])
    assert "pt2" not in capsys.readouterr().out and "pt2" not in seen[-1]
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-pt2"])
    assert "\tpt2 : True" in capsys.readouterr().out and seen[-1]["pt2"] is True


def test_switch_reaches_the_optimiser_and_the_summary(tmp_path, monkeypatch):
    import oracle_backend
    _b = _base()
    oracle_backend.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_b, "PartialSamplingOptimizer", FakeOptimizer)
    handed = []

    def grab(*a, **kw):
        handed.append(kw)
        raise Reached()

    monkeypatch.setattr(_b, "_summarise", grab)
    FakeOptimizer.calls.clear()
    with pytest.raises(Reached):
        _b.run(n_hid=128, argv=COMMON + ["-o", str(tmp_path / "off")])
    assert FakeOptimizer.calls == [("solve_H", 1234)] and "pt2" not in handed[-1]
    FakeOptimizer.calls.clear()
    with pytest.raises(Reached):
        _b.run(n_hid=128, argv=COMMON + ["-o", str(tmp_path / "on"), "-pt2"])
    assert FakeOptimizer.calls == [("solve_H_pt2", 1234)]            # one draw for both numbers
    assert handed[-1]["pt2"]["e_pt2"] == -1e-3 and handed[-1]["pt2"]["n_external"] == 150


def test_summary_lines(tmp_path, capsys):
    _b = _base()
    from naqs_amd.optimizer import LogKey
    opt = types.SimpleNamespace(log={LogKey.E_LOC: [(0, -7.4), (1, -7.45)]}, n_steps=2, save_loc=str(tmp_path / "s"),
                                save_log=lambda quiet=True: None)
    mol = types.SimpleNamespace(name="LiH", fci_energy=-7.51, hf_energy=-7.4, ccsd_energy=-7.5)
    plain = _b._summarise(opt, mol, "x", -7.5, 40, 1.0)
    text_plain = open(tmp_path / "s" / "summary.txt").read()
    assert "PT2" not in text_plain and "e_pt2" not in plain
    res = _b._summarise(opt, mol, "x", -7.5, 40, 1.0, pt2=dict(e_pt2=-9e-3, n_external=150, n_intruders=0))
    lines = open(tmp_path / "s" / "summary.txt").read().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("sampled-subspace diagonalisation (40 states) : ")][0]
    assert lines[at + 1] == ("sampled-subspace diagonalisation + Epstein-Nesbet PT2 (150 connected states) : -7.50900000 "
                             "(error to FCI 1.0000 mHa)")
    assert res["e_pt2"] == -9e-3 and res["eig"] == -7.5
    assert [ln for ln in lines if ln not in (lines[at + 1],)] == text_plain.splitlines()       # nothing else moves
    _b._summarise(opt, mol, "x", -7.5, 40, 1.0, pt2=dict(e_pt2=-9e-3, n_external=150, n_intruders=3))
    lines = open(tmp_path / "s" / "summary.txt").read().splitlines()
    assert lines[at + 2] == "PT2 : 3 states at or above the subspace energy left out"
    mol.fci_energy = None
    _b._summarise(opt, mol, "x", -7.5, 40, 1.0, pt2=dict(e_pt2=-9e-3, n_external=150, n_intruders=0))
    lines = open(tmp_path / "s" / "summary.txt").read().splitlines()
    assert lines[at + 1].endswith("(150 connected states) : -7.50900000")
    capsys.readouterr()
