"""``naqs_net_sr_solve`` (the natural-gradient step's two Cholesky solves in the library), the parts that need no GPU: the C-ABI
surface of the entry, the optimiser's ``solver`` key, the ``-sr_solver`` switch of the command line, and a rehearsal of the
error measures of tests/sr_solve_reference.py on its float64 blocked model (tests/test_sr_solve_gpu.py holds the kernels to them)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import sr_solve_reference as ss
from conftest import GOLDEN, PKG, ROOT
from naqs_amd import _lib

torch = pytest.importorskip("torch")
LIH = os.path.join(GOLDEN, "ham_LiH.npz")


def test_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "naqs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint naqs_net_sr_solve\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 10
    res, args = _lib.SIGNATURES["naqs_net_sr_solve"]
    assert res is ctypes.c_int and len(args) == 10
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "naqs_net_sr_solve")
    assert "int32_t *info_dev" in code and "cholesky_ex" in header
    # an addition: the version every earlier client checks is unchanged
    assert int(re.search(r"#define NAQS_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.load_library().naqs_abi_version() == 9


def test_entry_point_refuses_a_null_handle():
    assert _lib.load_library().naqs_net_sr_solve(None, 1, None, None, None, None, None, None, None, None) == -1


def test_solver_key_is_validated():
    from naqs_amd.optimizer import PartialSamplingOptimizer
    for bad in (dict(diag_shift=1e-3, lr=0.1, solver="x"), dict(diag_shift=1e-3, lr=0.1, solver=None),
                dict(diag_shift=1e-3, lr=0.1, solver="hip", x=1), dict(lr=0.1, solver="hip")):
        with pytest.raises(ValueError, match="natural_gradient"):
            PartialSamplingOptimizer(n_samples=10, natural_gradient=bad)
    # the accepted forms get past the check (and fail later, on the arguments this call leaves out)
    for good in (dict(diag_shift=1e-3, lr=0.1), dict(diag_shift=1e-3, lr=0.1, solver="torch"), dict(diag_shift=1e-3, lr=0.1, solver="hip")):
        with pytest.raises(Exception) as got:
            PartialSamplingOptimizer(n_samples=10, natural_gradient=good)
        assert "natural_gradient" not in str(got.value)


def test_absent_solver_key_is_the_torch_solve(monkeypatch):
    """The step with the key absent and with "torch" calls torch's Cholesky and never ``sr_solve``; with "hip" the reverse."""
    from naqs_amd.optimizer import PartialSamplingOptimizer
    eye = torch.eye(3, dtype=torch.float64)

    class Fused:
        def __init__(self):
            self.calls = []

        def sr_gram(self, saved, w, g, shift):
            return 4 * eye, 16 * eye, torch.ones(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)

        def sr_solve(self, Ta, Tp, ya, yp):
            self.calls.append("sr_solve")
            return ya / 4, yp / 16, torch.zeros(2, dtype=torch.int32)

        def sr_direction(self, saved, w, xa, xp):
            self.calls.append((xa.tolist(), xp.tolist()))
            return torch.zeros(1)

    class Wf:
        def flatten_parameters(self):
            return torch.zeros(1)

    seen = {}
    for how, ng in (("absent", dict(diag_shift=1e-3, lr=0.1)), ("torch", dict(diag_shift=1e-3, lr=0.1, solver="torch")),
                    ("hip", dict(diag_shift=1e-3, lr=0.1, solver="hip"))):
        opt = object.__new__(PartialSamplingOptimizer)
        opt.natural_gradient, opt.wavefunction = ng, Wf()
        fused = Fused()
        opt._natural_gradient_update(fused, None, None, None)
        seen[how] = fused.calls
        assert opt.sr_last["solver"] == ("hip" if how == "hip" else "torch") and opt.sr_last["M"] == 3
    assert seen["absent"] == seen["torch"] == [([0.25] * 3, [0.0625] * 3)]
    assert seen["hip"] == ["sr_solve", ([0.25] * 3, [0.0625] * 3)]


def _base():
    sys.path.insert(0, PKG)
    from experiments import _base
    return _base


def test_parser_accepts_sr_solver_and_lists_it_only_when_given(monkeypatch, capsys):
    _b = _base()
    p = _b.get_parser(n_hid=128)
    assert p.parse_args("-m molecules/LiH -sr".split()).sr_solver is None
    assert p.parse_args("-m molecules/LiH -sr -sr_solver hip".split()).sr_solver == "hip"
    assert p.parse_args("-m molecules/LiH -sr -sr_solver torch".split()).sr_solver == "torch"
    with pytest.raises(SystemExit):
        p.parse_args("-m molecules/LiH -sr -sr_solver lapack".split())
    capsys.readouterr()
    seen = []
    monkeypatch.setattr(_b, "_run", lambda **kw: seen.append(kw) or [])
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-sr"])
    assert "sr_solver" not in capsys.readouterr().out and "sr_solver" not in seen[-1]
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-sr", "-sr_solver", "hip"])
    assert "\tsr_solver : hip" in capsys.readouterr().out and seen[-1]["sr_solver"] == "hip" and seen[-1]["sr"] is True


def test_sr_solver_without_sr_is_refused(tmp_path):
    _b = _base()
    with pytest.raises(ValueError, match="-sr_solver .* -sr"):
        _b.run(n_hid=16, argv=["-m", LIH, "-o", str(tmp_path / "run"), "-s", "7", "-sr_solver", "hip"])


def test_switch_reaches_the_optimiser(tmp_path, monkeypatch):
    import oracle_backend
    _b = _base()
    oracle_backend.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    class Reached(Exception):
        pass

    def grab(**kw):
        raise Reached(kw.get("natural_gradient"))

    monkeypatch.setattr(_b, "PartialSamplingOptimizer", grab)
    common = ["-m", LIH, "-o", str(tmp_path / "run"), "-single_phase", "-n_hid", "16", "-n_hid_phase", "32", "-n_train", "2", "-s", "7",
              "-sr", "-sr_shift", "1e-4", "-sr_lr", "0.05"]
    with pytest.raises(Reached) as got:
        _b.run(n_hid=128, argv=common)
    assert got.value.args[0] == dict(diag_shift=1e-4, lr=0.05) and "solver" not in got.value.args[0]
    with pytest.raises(Reached) as got:
        _b.run(n_hid=128, argv=common + ["-sr_solver", "hip"])
    assert got.value.args[0] == dict(diag_shift=1e-4, lr=0.05, solver="hip")


@pytest.mark.parametrize("M", ss.SIZES)
def test_blocked_model_meets_the_bounds(M):
    """Rehearsal of the measures: the float64 blocked model of the kernels' algorithm, and LAPACK itself, sit inside the three
    bounds on the generator's systems; a float32 rounding of the solution does not."""
    for shift in ss.SHIFTS:
        for T, y in ss.pair(M, shift):
            x_ref, info_ref = ss.lapack_solve(T, y)
            x, L, info = ss.blocked_model(T, y)
            assert info == info_ref == 0
            cond = np.linalg.cond(T)
            for xs in (x, x_ref):
                assert ss.eta(T, xs, y) <= ss.bound(M), (M, shift)
            assert ss.rho(T, L) <= ss.bound(M) and ss.fwd(x, x_ref) <= cond * ss.bound(M), (M, shift)
            if M >= 63:
                assert ss.eta(T, x.astype(np.float32), y) > ss.bound(M), (M, shift)


def test_blocked_model_reports_the_pivot_like_lapack():
    (T, y), _ = ss.pair(200, 1e-3)
    for p in (0, 5, 63, 64, 65, 130, 199):
        Tb = T.copy()
        Tb[p, p] = -1.0
        x, _, info = ss.blocked_model(Tb, y)
        assert info == ss.lapack_solve(Tb, y)[1] == p + 1 and np.isnan(x).all()
    Tb = T.copy()
    Tb[64, 64] = np.nan
    assert ss.blocked_model(Tb, y)[2] == 65
