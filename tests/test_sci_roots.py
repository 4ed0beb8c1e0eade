"""Selected CI for several roots without a GPU: the preconditions of the schedules tests/test_sci_roots_gpu.py runs on the device,
checked on the dense reference loop of tests/sci_roots_reference.py at every growth step —

* ``sci_reference.cuts_are_clear`` with its own 1e-6 / 1e-12: nothing near a cut but tau's own group;
* every gap between consecutive roots, and from the last root to the first one left out, at least 1e-3 Ha (the roots are the
  K lowest of each subspace, none is followed: a crossing would swap them between the device and the reference);
* no denominator |diag_a - e_j| of a live root below 1e-6 (a row whose intruder status the two sides could decide differently)

— the averaged rule's consequences (one root with weight 1 is the single-root rule; a weight of 0 takes its root out), the
C-ABI surface of the two new entry points, the Python argument checks that need no device, the ``-sci_roots`` switch from the
command line to the optimiser and into summary.txt.

A schedule that is NOT run, and why: H2O with 2 roots from its two lowest determinants, steps (2, 4, 8, 16, 32), grows
M = 2 -> 4 -> 9 -> 17 -> 33 -> 66 with gaps >= 6.4e-2 and clear cuts, but at iteration 0 the two determinants do not couple, root 1
IS the second determinant (0x6ff), and its spin partner 0x9ff outside the subspace has the same H_aa to the bit: den = 0.0
exactly, with num = -0.038.  The dense loop calls that row an intruder; a solver whose e_1 is off by one rounding calls it a
row of importance ~1e11.  ``test_h2o_with_two_roots_meets_a_zero_denominator`` holds the figures; H2O runs with 3 roots on the
same steps instead (both partners inside from the start: min |den| 4.5e-2)."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

import sci_reference as sci
import sci_roots_reference as R
from conftest import GOLDEN, PKG, ROOT
from naqs_amd import _lib

torch = pytest.importorskip("torch")

LIH = os.path.join(GOLDEN, "ham_LiH.npz")
SIZES = {"LiH": [3, 6, 13, 26, 50], "H2O": [3, 5, 10, 18, 34, 67], "N2": [3, 7, 15, 31, 64, 129]}


# ---- the schedules' preconditions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol", sorted(R.SCHEDULES_ROOTS))
def test_schedules_meet_their_preconditions(mol):
    n_roots, n_add = R.SCHEDULES_ROOTS[mol]
    res = R.dense_run(mol)
    hist = res["history"]
    print(f"{mol} {n_roots} roots: M {[h['M'] for h in hist]}, external {[h['n_external'] for h in hist]}, smallest gap {min(R.gaps(hist)):.2e}, "
          f"smallest |den| {min(h['min_den'] for h in hist):.2e}")
    assert res["stopped"] == "schedule" and [h["M"] for h in hist] == SIZES[mol] and len(hist) == len(n_add) + 1
    assert sci.cuts_are_clear(hist) == []
    assert sum(h["cut"] is not None for h in hist) >= len(n_add) - 1
    assert all(g >= 1e-3 for g in R.gaps(hist))
    assert all(h["min_den"] >= 1e-6 for h in hist)
    assert all(n == 0 for h in hist for n in h["n_intruders"]) and all(p < 0 for h in hist for p in h["e_pt2"])
    # nested subspaces: no root ever rises; every root stays above the sector's own
    for a, b in zip(hist, hist[1:]):
        assert all(y <= x + 1e-12 for x, y in zip(a["e0"], b["e0"]))
    assert len(np.unique(res["keys"])) == len(res["keys"]) == hist[-1]["M"]
    assert np.abs(res["vecs"] @ res["vecs"].T - np.eye(n_roots)).max() <= 1e-12


def test_h2o_with_two_roots_meets_a_zero_denominator():
    packed, fci, k0 = R.start("H2O", 2)
    assert [int(k) for k in k0] == [0x3ff, 0x6ff]
    hist = R.loop(packed, k0, 2, (2, 4, 8, 16, 32))["history"]
    assert [h["M"] for h in hist] == [2, 4, 9, 17, 33, 66] and min(R.gaps(hist)) >= 6e-2 and sci.cuts_are_clear(hist) == []
    assert hist[0]["min_den"] == 0.0 and hist[0]["n_intruders"] == [0, 1] and all(h["min_den"] > 0.1 for h in hist[1:])


def test_start_takes_the_lowest_determinants_in_order():
    for mol, (n_roots, _) in R.SCHEDULES_ROOTS.items():
        packed, fci, k0 = R.start(mol, n_roots)
        d = sci.diagonal(packed, k0)
        assert len(k0) == n_roots == len(np.unique(k0)) and np.all(np.diff(d) >= 0)
        assert k0[0] == sci.start(mol)[2][0]


# ---- the averaged rule --------------------------------------------------------------------------------------------------------
def _rows(n, nb, seed):
    rs = np.random.RandomState(seed)
    keys = (rs.permutation(4 * n)[:n].astype(np.uint64) + np.uint64(5)) << np.uint64(2)
    return keys, rs.normal(size=(nb, n)), rs.lognormal(size=n), -rs.lognormal(size=nb)


def test_one_root_of_weight_one_is_the_single_root_rule():
    keys, num, diag, e = _rows(300, 1, 1)
    num[0, ::7] = np.round(num[0, ::7], 1)
    diag[::7] = 0.5
    diag[::11] = e[0] - 0.25                     # intruders
    num[0, 5] = np.nan
    for k in (0, 1, 17, 150, 299, 300, 500):
        for kw in (dict(), dict(tie_rtol=0.0), dict(eps_min=0.3)):
            one = sci.select(keys, num[0], diag, e[0], k, **kw)
            avg = R.select(keys, num, diag, e, [1.0], k, **kw)
            assert np.array_equal(one[0], avg[0]) and one[1] == avg[1]
            assert np.array_equal(one[2]["eps"], avg[2]["eps"], equal_nan=True)


def test_a_weight_of_zero_takes_its_root_out():
    keys, num, diag, e = _rows(200, 3, 2)
    num[1] = np.nan                               # never read: not even its NaNs and its energy count
    e[:] = (-10.0, np.inf, -0.1)
    diag[::9] = e[2] - 0.5                        # intruders of root 2 only: den = 9.4 for root 0
    for k in (1, 20, 200):
        one = sci.select(keys, num[0], diag, e[0], k)
        avg = R.select(keys, num, diag, e, [1.0, 0.0, 0.0], k)
        assert np.array_equal(one[0], avg[0]) and one[1] == avg[1] and one[1][1] == 0
        two = R.select(keys, num, diag, e, [0.5, 0.0, 0.5], k)
        assert two[1][1] > 0 and np.all(np.isinf(two[2]["eps"][::9]))      # an intruder of any live root is one


def test_rule_sums_the_roots_in_order_one_rounding_each():
    num = np.array([[3.0, 1.0], [1.0, 2.0], [0.1, 0.7]])
    diag, e, w = np.array([1.0, 2.0]), np.array([0.0, -1.0, -2.0]), np.array([0.2, 0.3, 0.5])
    eps = R.importance(num, diag, e, w)[0]
    for a in range(2):
        want = w[0] * ((num[0, a] * num[0, a]) / (diag[a] - e[0]))
        want = want + w[1] * ((num[1, a] * num[1, a]) / (diag[a] - e[1]))
        want = want + w[2] * ((num[2, a] * num[2, a]) / (diag[a] - e[2]))
        assert eps[a] == want
    assert np.array_equal(R.equal_weights(3), np.full(3, 1.0 / 3.0))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "naqs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert int(re.search(r"#define NAQS_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 9      # additions
    lib = _lib.load_library()
    m = re.search(r"\bint naqs_ham_pt2_block\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 12
    for arg in ("int64_t M", "const uint64_t *keys_dev", "int32_t nb", "const double *C_dev", "const double *e_host", "int64_t n_ext",
                "const uint64_t *ext_keys_dev", "double *num_dev", "double *diag_dev", "double *out4_dev", "void *stream"):
        assert arg in m.group(1)
    res, args = _lib.SIGNATURES["naqs_ham_pt2_block"]
    assert res is ctypes.c_int and len(args) == 12 and args[3] is ctypes.c_int32
    m = re.search(r"\bint naqs_ham_pt2_select_avg\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 15
    for arg in ("int64_t n_ext", "const uint64_t *ext_keys_dev", "int32_t nb", "const double *num_dev", "const double *diag_dev",
                "const double *e_host", "const double *w_host", "int64_t k", "double eps_min", "double tie_rtol", "int64_t capacity",
                "uint64_t *out_keys_dev", "int64_t *count_dev"):
        assert arg in m.group(1)
    res, args = _lib.SIGNATURES["naqs_ham_pt2_select_avg"]
    assert res is ctypes.c_int and len(args) == 15 and [i for i, a in enumerate(args) if a is ctypes.c_double] == [9, 10]
    raw = ctypes.CDLL(_lib.lib_path())
    assert hasattr(raw, "naqs_ham_pt2_block") and hasattr(raw, "naqs_ham_pt2_select_avg")
    one = (ctypes.c_double * 1)(1.0)
    assert lib.naqs_ham_pt2_block(None, 1, None, 1, None, one, 0, None, None, None, None, None) == -1
    assert lib.naqs_ham_pt2_select_avg(None, 0, None, 1, None, None, one, one, 1, 0.0, 0.0, 0, None, None, None) == -1


# ---- Python argument checks that need no device -------------------------------------------------------------------------------
def _bare_ham():
    from naqs_amd.hamiltonian import DevicePauliHamiltonian
    ham = object.__new__(DevicePauliHamiltonian)
    ham.device = torch.device("cpu")
    ham._h = None                                 # close() in __del__ finds nothing to free
    return ham


def test_python_refuses_before_any_launch():
    ham = _bare_ham()
    keys = torch.arange(5, dtype=torch.int64)
    for n_roots in (0, 9, -1):
        with pytest.raises(ValueError, match="n_roots must lie in 1..8"):
            ham.selected_ci_roots(keys, n_roots, (1, 2))
    with pytest.raises(ValueError, match="5 keys cannot carry 6 roots"):
        ham.selected_ci_roots(keys, 6, (1, 2))
    with pytest.raises(ValueError, match="int64 device tensors"):
        ham.pt2_block(keys, torch.zeros((2, 5), dtype=torch.float64), [0.0, 0.0], keys)
    with pytest.raises(ValueError, match="int64 device tensor"):
        ham.pt2_select_roots(keys, torch.zeros((2, 5), dtype=torch.float64), torch.zeros(5, dtype=torch.float64), [0.0, 0.0], 1)


def test_solve_h_roots_sci_needs_a_device_and_a_root_count():
    from naqs_amd.optimizer import PartialSamplingOptimizer
    opt = object.__new__(PartialSamplingOptimizer)
    opt.device = torch.device("cpu")
    with pytest.raises(NotImplementedError, match="solve_H_roots_sci"):
        opt.solve_H_roots_sci(n_samps=10, n_roots=2, n_iter=3)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="n_roots must lie in 1..8"):
            opt.solve_H_roots_sci(n_samps=10, n_roots=bad)


# ---- the command line ---------------------------------------------------------------------------------------------------------
def _base():
    sys.path.insert(0, PKG)
    from experiments import _base
    return _base


class Reached(Exception):
    pass


GROWN = dict(keys=None, vecs=None, eigs=[-7.52, -7.41], stopped="schedule", extrapolated=[-7.6, None], n_unq=40,
             history=[dict(M=30, e0=[-7.5, -7.4], e_pt2=[-9e-3, -8e-3], n_external=150, n_intruders=[0, 0], n_added=30),
                      dict(M=60, e0=[-7.52, -7.41], e_pt2=[-1e-3, -2e-3], n_external=120, n_intruders=[0, 0], n_added=0)])
ROOTS = dict(keys=None, eigs=[-7.5, -7.4], vec0s=[0.9, 0.1], n_unq=40)


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

    def solve_H_sci(self, n_samps=None, **kw):
        FakeOptimizer.calls.append(("solve_H_sci", n_samps, kw))
        return dict(keys=None, vec=None, stopped="schedule", extrapolated=None, n_unq=40,
                    history=[dict(M=30, e0=-7.5, e_pt2=-9e-3, n_external=150, n_intruders=0, n_added=0)])

    def solve_H_roots(self, n_samps=None, **kw):
        FakeOptimizer.calls.append(("solve_H_roots", n_samps, kw))
        return ROOTS

    def solve_H_roots_sci(self, n_samps=None, **kw):
        FakeOptimizer.calls.append(("solve_H_roots_sci", n_samps, kw))
        return GROWN


COMMON = ["-m", LIH, "-single_phase", "-n_hid", "16", "-n_hid_phase", "32", "-n_train", "2", "-s", "7", "-lr", "0.001"]


@pytest.mark.parametrize("extra", [[], ["-roots", "2"], ["-sci", "3"], ["-roots", "2", "-sci", "0"]])
def test_the_switch_needs_roots_and_sci(extra):
    _b = _base()
    with pytest.raises(ValueError, match="give -roots and -sci as well"):
        _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-sci_roots"] + extra)
    roots = 2 if "-roots" in extra else None
    sci_n = 3 if extra == ["-sci", "3"] else 0
    with pytest.raises(ValueError, match="give -roots and -sci as well"):
        _b._check_sci_roots(True, roots, sci_n)                         # _run's own guard
    _b._check_sci_roots(False, roots, sci_n)
    _b._check_sci_roots(True, 2, 3)


def test_parser_lists_the_switch_only_when_given(monkeypatch, capsys):
    _b = _base()
    p = _b.get_parser(n_hid=128)
    assert p.parse_args("-m molecules/LiH".split()).sci_roots is False
    assert p.parse_args("-m molecules/LiH -roots 2 -sci 3 -sci_roots".split()).sci_roots is True
    seen = []
    monkeypatch.setattr(_b, "_run", lambda **kw: seen.append(kw) or [])
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-roots", "2", "-sci", "3"])
    assert "sci_roots" not in capsys.readouterr().out and "sci_roots" not in seen[-1]
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-roots", "2", "-sci", "3", "-sci_roots"])
    assert "\tsci_roots : True" in capsys.readouterr().out and seen[-1]["sci_roots"] is True and seen[-1]["roots"] == 2 and seen[-1]["sci"] == 3


def test_switch_reaches_the_optimiser_and_the_summary(tmp_path, monkeypatch):
    import oracle_backend
    _b = _base()
    oracle_backend.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_b, "PartialSamplingOptimizer", FakeOptimizer)
    handed = []

    def grab(*a, **kw):
        handed.append((a, kw))
        raise Reached()

    monkeypatch.setattr(_b, "_summarise", grab)
    FakeOptimizer.calls.clear()
    with pytest.raises(Reached):
        _b.run(n_hid=128, argv=COMMON + ["-o", str(tmp_path / "off"), "-roots", "2", "-sci", "3"])
    assert [c[0] for c in FakeOptimizer.calls] == ["solve_H_sci", "solve_H_roots"] and "roots_sci" not in handed[-1][1]
    assert handed[-1][1]["roots"] is ROOTS
    FakeOptimizer.calls.clear()
    with pytest.raises(Reached):
        _b.run(n_hid=128, argv=COMMON + ["-o", str(tmp_path / "on"), "-roots", "2", "-sci", "3", "-sci_grow", "0.5", "-sci_start", "30", "-sci_roots"])
    # the roots' stage is the grown one, on its own draw, behind the ground state's -sci; no solve_H_roots beside it
    assert FakeOptimizer.calls == [("solve_H_sci", 1234, dict(n_iter=3, grow=0.5, n_start=30)),
                                   ("solve_H_roots_sci", 1234, dict(n_roots=2, n_iter=3, grow=0.5, n_start=30))]
    kw = handed[-1][1]
    # iteration 0 feeds today's lines; with -sci_start they say the cut subspace's size, not the draw's
    assert kw["roots_sci"] is GROWN and kw["roots"] == dict(eigs=[-7.5, -7.4], n_unq=30)
    with pytest.raises(Reached):
        _b.run(n_hid=128, argv=COMMON + ["-o", str(tmp_path / "pt2"), "-roots", "2", "-sci", "2", "-sci_roots", "-pt2"])
    assert handed[-1][1]["roots"] == dict(eigs=[-7.5, -7.4], n_unq=40, e_pt2=[-9e-3, -8e-3])


def test_summary_lines(tmp_path, capsys):
    _b = _base()
    from naqs_amd.optimizer import LogKey
    opt = types.SimpleNamespace(log={LogKey.E_LOC: [(0, -7.4), (1, -7.45)]}, n_steps=2, save_loc=str(tmp_path / "s"),
                                save_log=lambda quiet=True: None)
    mol = types.SimpleNamespace(name="LiH", fci_energy=-7.51, hf_energy=-7.4, ccsd_energy=-7.5)
    plain = _b._summarise(opt, mol, "x", -7.5, 40, 1.0, roots=ROOTS)
    text_plain = open(tmp_path / "s" / "summary.txt").read().splitlines()
    assert not any(k.startswith("roots_sci") for k in plain) and not any("selected CI" in ln for ln in text_plain)
    res = _b._summarise(opt, mol, "x", -7.5, 40, 1.0, roots=ROOTS, roots_sci=GROWN)
    lines = open(tmp_path / "s" / "summary.txt").read().splitlines()
    assert lines[:len(text_plain)] == text_plain                                          # the new lines stand behind, nothing moves
    assert lines[len(text_plain):] == [
        "selected CI for 2 roots iteration 0 (30 states, 150 connected) : E -7.50000000 , -7.40000000",
        "selected CI for 2 roots iteration 1 (60 states, 120 connected) : E -7.52000000 , -7.41000000",
        "selected CI root 0 (60 states) : -7.52000000 , gap to root 0 0.0000 mHa , E + E_PT2 -7.52100000 , "
        "extrapolated to E_PT2 = 0 (non-variational) -7.60000000",
        "selected CI root 1 (60 states) : -7.41000000 , gap to root 0 110.0000 mHa , E + E_PT2 -7.41200000 , "
        "extrapolated to E_PT2 = 0 (non-variational) n/a",
        "selected CI for 2 roots stopped : schedule"]
    assert res["roots_sci_history"] == GROWN["history"] and res["roots_sci_stopped"] == "schedule" and res["roots"] == ROOTS["eigs"]
    assert res["roots_sci_eigs"] == GROWN["eigs"] and res["roots_sci_extrapolated"] == [-7.6, None]
    capsys.readouterr()
