"""Selected CI without a GPU: the dense reference loop of tests/sci_reference.py on the committed fixtures (nested subspaces, so
E_S never rises and never drops below FCI; LiH closes on its ground state's symmetry block), the precondition of the schedules
tests/test_sci_gpu.py runs on the device, the selection rule's edge cases, the C-ABI surface of ``naqs_ham_pt2_select``, the
``-sci`` flags from the command line to the optimiser and into summary.txt, and ``solve_H_sci``'s refusal without a device."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

import sci_reference as sci
from conftest import GOLDEN, PKG, ROOT
from naqs_amd import _lib

torch = pytest.importorskip("torch")

LIH = os.path.join(GOLDEN, "ham_LiH.npz")


@pytest.fixture(scope="module", params=["LiH", "H2O", "N2"])
def run(request):
    packed, fci, k0 = sci.start(request.param)
    return request.param, fci, sci.loop(packed, k0, sci.SCHEDULES[request.param])


# ---- the loop ---------------------------------------------------------------------------------------------------------------
def test_subspace_energy_never_rises_and_never_passes_fci(run):
    mol, fci, res = run
    e = [h["e0"] for h in res["history"]]
    for h in res["history"]:
        print(f"{mol} M={h['M']}: E_S - FCI {h['e0'] - fci:.3e}, E_S + E_PT2 - FCI {h['e0'] + h['e_pt2'] - fci:+.2e}")
    assert len(e) == len(sci.SCHEDULES[mol]) + 1 and res["stopped"] == "schedule"
    assert all(b <= a for a, b in zip(e, e[1:]))                     # nested subspaces (Cauchy interlacing)
    assert all(x >= fci - 1e-10 for x in e)
    assert all(h["e_pt2"] <= 0 and h["n_intruders"] == 0 for h in res["history"])
    assert len(np.unique(res["keys"])) == len(res["keys"]) == res["history"][-1]["M"]
    assert e[-1] - fci < 1e-2 * (e[0] - fci)


def test_schedules_cut_clear_of_every_other_importance(run):
    """The precondition of the device test's schedules: nothing within 1e-6 of a cut but tau's own group (within 1e-12)."""
    mol, fci, res = run
    assert sci.cuts_are_clear(res["history"]) == []
    assert sum(h["cut"] is not None for h in res["history"]) >= len(sci.SCHEDULES[mol]) - 1
    if mol == "N2":
        assert res["history"][-1]["M"] >= 256


def test_lih_schedule_ends_inside_a_degenerate_pair():
    packed, fci, k0 = sci.start("LiH")
    hist = sci.loop(packed, k0, sci.SCHEDULES["LiH"])["history"]
    assert [h["M"] for h in hist] == [1, 2, 4, 8, 16, 32, 65] and hist[-2]["n_added"] == 33 and hist[-2]["k"] == 32


def test_lih_closes_on_its_symmetry_block():
    packed, fci, k0 = sci.start("LiH")
    res = sci.loop(packed, k0, (1000,) * 8)
    last = res["history"][-1]
    assert res["stopped"] == "connected set empty" and last["n_external"] == 0 and last["M"] == 69
    assert abs(last["e0"] - fci) <= 1e-10 and last["e_pt2"] == 0.0


def test_grow_schedule_is_read_as_the_device_reads_it():
    from naqs_amd.hamiltonian import _sci_schedule
    assert _sci_schedule((1, 2, 4)) == ([1, 2, 4], None) and sci.schedule((1, 2, 4)) == ([1, 2, 4], None, 4)
    assert _sci_schedule((3, 1.0)) == (3, 1.0) and sci.schedule((3, 1.0)) == (None, 1.0, 3)
    assert _sci_schedule((3, 1)) == ([3, 1], None)                    # two ints are two growth steps
    with pytest.raises(ValueError):
        _sci_schedule((0, 1.0))
    with pytest.raises(ValueError):
        _sci_schedule((2, 0.0))
    packed, fci, k0 = sci.start("LiH")
    assert [h["M"] for h in sci.loop(packed, k0, (4, 1.0))["history"]] == [1, 2, 4, 8]


# ---- the rule ---------------------------------------------------------------------------------------------------------------
KEYS = np.arange(100, 108, dtype=np.uint64)


def _sel(num, diag, k, e0=-1.0, **kw):
    keys, counts, info = sci.select(KEYS[:len(num)], num, diag, e0, k, **kw)
    return list(keys - 100), counts


def test_rule_k_below_one_and_beyond_the_eligible():
    num, diag = [1.0, 2.0, 0.0, 3.0], [0.0, 0.0, 0.0, 0.0]
    assert _sel(num, diag, 0) == ([], (0, 0)) and _sel(num, diag, -3) == ([], (0, 0))
    assert _sel(num, diag, 1) == ([3], (1, 0)) and _sel(num, diag, 2) == ([1, 3], (2, 0))
    assert _sel(num, diag, 3) == ([0, 1, 3], (3, 0)) == _sel(num, diag, 4) == _sel(num, diag, 99)      # the zero never joins


def test_rule_all_equal_and_ties():
    assert _sel([2.0] * 5, [0.0] * 5, 1) == ([0, 1, 2, 3, 4], (5, 0))
    assert _sel([2.0] * 5, [0.0] * 5, 1, tie_rtol=0.0) == ([0, 1, 2, 3, 4], (5, 0))
    near = [2.0, 2.0 * (1 + 1e-12), 1.0]
    assert _sel(near, [0.0] * 3, 1) == ([0, 1], (2, 0))               # 2e-12 apart in eps: one group at 1e-9
    assert _sel(near, [0.0] * 3, 1, tie_rtol=0.0) == ([1], (1, 0))
    assert _sel([3.0, 2.0, 1.0], [0.0] * 3, 1, tie_rtol=0.6) == ([0, 1], (2, 0))      # 9, 4, 1 against a cut of 9 x 0.4
    assert _sel([3.0, 2.0, 1.0], [0.0] * 3, 1, tie_rtol=0.5) == ([0], (1, 0))


def test_rule_eps_min():
    num, diag = [1.0, 2.0, 3.0], [0.0] * 3
    assert _sel(num, diag, 3, eps_min=4.0) == ([1, 2], (2, 0))        # eps = 1, 4, 9; 4 >= 4 stays
    assert _sel(num, diag, 1, eps_min=4.0) == ([2], (1, 0))
    assert _sel(num, diag, 3, eps_min=10.0) == ([], (0, 0))


def test_rule_intruders_come_first_and_zeros_never():
    num = [1.0, 5.0, 0.0, float("nan"), 2.0, -0.0]
    diag = [0.0, -2.0, -2.0, 0.0, float("nan"), 0.0]                  # e0 = -1: rows 1, 2 have den < 0, row 4 a NaN den
    assert _sel(num, diag, 1) == ([1, 2, 3, 4], (4, 4))               # every intruder ties at +inf — even one with num = 0
    assert _sel(num, diag, 5) == ([0, 1, 2, 3, 4], (5, 4)) == _sel(num, diag, 6)
    assert _sel(num, diag, 4, eps_min=float("inf")) == ([1, 2, 3, 4], (4, 4))


def test_extrapolation_is_polyfits_intercept():
    from naqs_amd.hamiltonian import extrapolate_pt2
    hist = [dict(e0=-1.0, e_pt2=-0.3), dict(e0=-1.2, e_pt2=0.0), dict(e0=-1.25, e_pt2=-0.04), dict(e0=-1.27, e_pt2=-0.013),
            dict(e0=-1.28, e_pt2=-0.004)]
    assert extrapolate_pt2(hist[:3]) is None and extrapolate_pt2([]) is None
    want = np.polyfit([-0.04, -0.013, -0.004], [-1.25, -1.27, -1.28], 1)[1]
    assert extrapolate_pt2(hist) == pytest.approx(want, rel=1e-13)
    want4 = np.polyfit([-0.3, -0.04, -0.013, -0.004], [-1.0, -1.25, -1.27, -1.28], 1)[1]
    assert extrapolate_pt2(hist, n_fit=4) == pytest.approx(want4, rel=1e-13)
    packed, fci, k0 = sci.start("LiH")
    h = sci.loop(packed, k0, sci.SCHEDULES["LiH"])["history"]
    assert abs(extrapolate_pt2(h) - fci) < 1e-6


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "naqs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint naqs_ham_pt2_select\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 13
    for arg in ("int64_t n_ext", "const uint64_t *ext_keys_dev", "const double *num_dev", "const double *diag_dev", "double e0", "int64_t k",
                "double eps_min", "double tie_rtol", "int64_t capacity", "uint64_t *out_keys_dev", "int64_t *count_dev"):
        assert arg in m.group(1)
    res, args = _lib.SIGNATURES["naqs_ham_pt2_select"]
    assert res is ctypes.c_int and len(args) == 13 and [i for i, a in enumerate(args) if a is ctypes.c_double] == [5, 7, 8]
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "naqs_ham_pt2_select")
    assert int(re.search(r"#define NAQS_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 9      # an addition
    assert _lib.load_library().naqs_ham_pt2_select(None, 0, None, None, None, 0.0, 1, 0.0, 0.0, 0, None, None, None) == -1


# ---- the optimiser and the command line -------------------------------------------------------------------------------------
def test_solve_h_sci_needs_a_device():
    from naqs_amd.optimizer import PartialSamplingOptimizer
    opt = object.__new__(PartialSamplingOptimizer)
    opt.device = torch.device("cpu")
    with pytest.raises(NotImplementedError, match="solve_H_sci"):
        opt.solve_H_sci(n_samps=10, n_iter=3)


def _base():
    sys.path.insert(0, PKG)
    from experiments import _base
    return _base


class Reached(Exception):
    pass


SCI = dict(keys=None, vec=None, stopped="schedule", extrapolated=-7.6, n_unq=40,
           history=[dict(M=30, e0=-7.5, e_pt2=-9e-3, n_external=150, n_intruders=0, n_added=30),
                    dict(M=60, e0=-7.508, e_pt2=-1e-3, n_external=120, n_intruders=0, n_added=0)])


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
        return SCI


COMMON = ["-m", LIH, "-single_phase", "-n_hid", "16", "-n_hid_phase", "32", "-n_train", "2", "-s", "7", "-lr", "0.001"]


def test_parser_accepts_the_flags_and_lists_them_only_when_given(monkeypatch, capsys):
    _b = _base()
    p = _b.get_parser(n_hid=128)
    off = p.parse_args("-m molecules/LiH".split())
    assert off.sci == 0 and off.sci_grow is None and off.sci_start is None
    on = p.parse_args("-m molecules/LiH -sci 4 -sci_grow 0.5 -sci_start 20".split())
    assert on.sci == 4 and on.sci_grow == 0.5 and on.sci_start == 20
    seen = []
    monkeypatch.setattr(_b, "_run", lambda **kw: seen.append(kw) or [])
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7"])
    assert "\tsci" not in capsys.readouterr().out and not any(k.startswith("sci") for k in seen[-1])
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-sci", "3"])
    out = capsys.readouterr().out
    assert "\tsci : 3" in out and "sci_grow" not in out and "sci_start" not in out
    assert seen[-1]["sci"] == 3 and "sci_grow" not in seen[-1] and "sci_start" not in seen[-1]
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-sci", "3", "-sci_grow", "2.0", "-sci_start", "5"])
    out = capsys.readouterr().out
    assert "\tsci_grow : 2.0" in out and "\tsci_start : 5" in out and seen[-1]["sci_grow"] == 2.0 and seen[-1]["sci_start"] == 5


@pytest.mark.parametrize("extra", [["-sci_grow", "2.0"], ["-sci_start", "5"], ["-sci", "0", "-sci_grow", "2.0"]])
def test_growth_and_start_need_the_switch(extra):
    _b = _base()
    with pytest.raises(ValueError, match="give -sci as well"):
        _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7"] + extra)
    with pytest.raises(ValueError, match="give -sci as well"):
        _b._check_sci(0, 2.0 if "-sci_grow" in extra else None, 5 if "-sci_start" in extra else None)     # _run's own guard


def test_flags_reach_the_optimiser_and_the_summary(tmp_path, monkeypatch):
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
        _b.run(n_hid=128, argv=COMMON + ["-o", str(tmp_path / "off")])
    assert FakeOptimizer.calls == [("solve_H", 1234)] and "sci" not in handed[-1][1]
    FakeOptimizer.calls.clear()
    with pytest.raises(Reached):
        _b.run(n_hid=128, argv=COMMON + ["-o", str(tmp_path / "on"), "-sci", "3", "-sci_start", "30"])
    assert FakeOptimizer.calls == [("solve_H_sci", 1234, dict(n_iter=3, grow=1.0, n_start=30))]         # one draw, no solve_H beside it
    a, kw = handed[-1]
    assert kw["sci"] is SCI and "pt2" not in kw and a[3] == -7.5 and a[4] == 40       # iteration 0 feeds the existing lines
    with pytest.raises(Reached):
        _b.run(n_hid=128, argv=COMMON + ["-o", str(tmp_path / "both"), "-sci", "2", "-sci_grow", "0.5", "-pt2"])
    assert FakeOptimizer.calls[-1] == ("solve_H_sci", 1234, dict(n_iter=2, grow=0.5, n_start=None))
    assert handed[-1][1]["pt2"]["e_pt2"] == -9e-3 and handed[-1][1]["pt2"]["n_external"] == 150


def test_sci_on_the_cpu_is_refused(tmp_path, monkeypatch):
    """-sci with the real optimiser and no device: solve_H_sci raises, nothing falls back."""
    import oracle_backend
    _b = _base()
    oracle_backend.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(NotImplementedError, match="solve_H_sci"):
        _b.run(n_hid=128, argv=COMMON + ["-n_samps", "1000", "-n_unq_samps_min", "10", "-o", str(tmp_path / "cpu"), "-sci", "2"])


def test_summary_lines(tmp_path, capsys):
    _b = _base()
    from naqs_amd.optimizer import LogKey
    opt = types.SimpleNamespace(log={LogKey.E_LOC: [(0, -7.4), (1, -7.45)]}, n_steps=2, save_loc=str(tmp_path / "s"),
                                save_log=lambda quiet=True: None)
    mol = types.SimpleNamespace(name="LiH", fci_energy=-7.51, hf_energy=-7.4, ccsd_energy=-7.5)
    plain = _b._summarise(opt, mol, "x", -7.5, 40, 1.0)
    text_plain = open(tmp_path / "s" / "summary.txt").read()
    assert "selected CI" not in text_plain and not any(k.startswith("sci") for k in plain)
    res = _b._summarise(opt, mol, "x", -7.5, 40, 1.0, sci=SCI)
    lines = open(tmp_path / "s" / "summary.txt").read().splitlines()
    assert lines[:len(text_plain.splitlines())] == text_plain.splitlines()                   # the new lines stand behind, nothing moves
    new = lines[len(text_plain.splitlines()):]
    assert new == ["selected CI iteration 0 (30 states, 150 connected) : E_S -7.50000000 , E_S + E_PT2 -7.50900000 "
                   "(errors to FCI 10.0000 , 1.0000 mHa)",
                   "selected CI iteration 1 (60 states, 120 connected) : E_S -7.50800000 , E_S + E_PT2 -7.50900000 "
                   "(errors to FCI 2.0000 , 1.0000 mHa)",
                   "selected CI extrapolated to E_PT2 = 0 (non-variational) : -7.60000000 (error to FCI -90.0000 mHa)",
                   "selected CI stopped : schedule"]
    assert "PT2 (" not in "\n".join(lines)                                                      # that line is -pt2's
    assert res["sci_history"] == SCI["history"] and res["sci_stopped"] == "schedule" and res["eig"] == -7.5
    mol.fci_energy = None
    _b._summarise(opt, mol, "x", -7.5, 40, 1.0, sci=dict(SCI, extrapolated=None))
    lines = open(tmp_path / "s" / "summary.txt").read().splitlines()
    assert lines[-3].endswith("E_S + E_PT2 -7.50900000") and lines[-1] == "selected CI stopped : schedule"
    assert not any("extrapolated" in ln for ln in lines)
    capsys.readouterr()
