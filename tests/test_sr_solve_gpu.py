"""``naqs_net_sr_solve`` on the MI355X: the blocked float64 Cholesky solve of the natural-gradient step's two systems
(csrc/naqs_sr_solve.hip) against the measures and bounds of tests/sr_solve_reference.py.

1. Against float64: M in {2, 3, 63, 64, 65, 127, 128, 129, 200, 333, 777} (below, at and above one and two block edges, a ragged
   last block, 13 block columns) x shift in {1e-2, 1e-3, 1e-6}, systems a and phi from different seeds in one call, and M = 1:
   info = [0, 0], eta, rho <= max(M, 16) u, fwd <= cond_2 max(M, 16) u against LAPACK on the CPU, x finite.
2. Bits: the same call twice, a system alone and beside another, the systems swapped between the slots.
3. Failure is a status: a pivot made -1 or NaN -> info = [p + 1, 0] (LAPACK's own answer), x all NaN, the other system bit-equal.
4. Refusals.
5. The real systems: sr_gram -> sr_solve -> sr_direction on every case of sr_reference.CASES against the float64 direction, to
   the bounds the torch solve is held to (test_sr_gpu.C2_YARDSTICK).
6. The optimiser with solver="hip": no torch Cholesky is called, "torch" / absent never call sr_solve and agree bit for bit,
   100 steps on LiH end below Adam, a failed factorisation raises NaturalGradientError and leaves the parameters alone.
"""
import numpy as np
import pytest

import grad_reference as gr
import sr_reference as sr
import sr_solve_reference as ss
from naqs_amd.hamiltonian import _stream_ptr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_NET = {}
_SYS = {}


def _fused():
    """A handle that only serves as a device: no training forward is ever run on it."""
    if "fused" not in _NET:
        _, wf = gr.sector_net("LiH", amp_hidden=16, phase_hidden=(32,))
        _NET["wf"], _NET["fused"] = wf, wf.fused(need_phase=True)
        assert _NET["fused"] is not None
    return _NET["fused"]


def _pair(M, shift):
    """Per (M, shift), computed once and left unchanged: both systems, LAPACK's solutions on the CPU and cond_2."""
    if (M, shift) not in _SYS:
        out = []
        for T, y in ss.pair(M, shift):
            x_ref, info = ss.lapack_solve(T, y)
            assert info == 0
            out.append(dict(T=T, y=y, x_ref=x_ref, cond=float(np.linalg.cond(T))))
        _SYS[(M, shift)] = out
    return _SYS[(M, shift)]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _solve(Ta, ya, Tp=None, yp=None):
    """Fresh device copies -> numpy (x_a, x_phi, L_a, L_phi, info); the L are the returned matrices' lower triangles."""
    da, dp = _dev(Ta), (None if Tp is None else _dev(Tp))
    xa, xp, info = _fused().sr_solve(da, dp, _dev(ya), None if yp is None else _dev(yp))
    torch.cuda.synchronize()
    low = lambda t: None if t is None else np.tril(t.cpu().numpy())
    return xa.cpu().numpy(), None if xp is None else xp.cpu().numpy(), low(da), low(dp), info.cpu().numpy()


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ------------------------------------------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("M", ss.SIZES)
def test_solve_against_float64(M):
    worst = dict(eta=0.0, rho=0.0, fwd=0.0)
    for shift in ss.SHIFTS:
        a, p = _pair(M, shift)
        xa, xp, La, Lp, info = _solve(a["T"], a["y"], p["T"], p["y"])
        assert info.tolist() == [0, 0], (M, shift, info)
        for s, x, L in ((a, xa, La), (p, xp, Lp)):
            assert np.isfinite(x).all(), (M, shift)
            e, r, f = ss.eta(s["T"], x, s["y"]), ss.rho(s["T"], L), ss.fwd(x, s["x_ref"]) / (s["cond"] * ss.U)
            worst = dict(eta=max(worst["eta"], e), rho=max(worst["rho"], r), fwd=max(worst["fwd"], f))
            print(f"\n[sr solve] M={M} shift={shift:g}: eta {e:.3e} rho {r:.3e} (bound {ss.bound(M):.2e}), fwd / (cond u) {f:.3e} "
                  f"(bound {max(M, 16)}), cond {s['cond']:.2e}", end="")
            assert e <= ss.bound(M) and r <= ss.bound(M) and f <= max(M, 16), (M, shift, e, r, f)
    print(f"\n[sr solve] M={M}: worst eta {worst['eta']:.3e}, rho {worst['rho']:.3e}, fwd / (cond u) {worst['fwd']:.3e}")


@pytest.mark.parametrize("t", [2.5, 1e-300])
def test_one_by_one(t):
    T, y = np.array([[t]]), np.array([0.75 * t])
    xa, xp, La, Lp, info = _solve(T, y, 4 * T, -y)
    assert info.tolist() == [0, 0]
    assert La[0, 0] == np.sqrt(t) and Lp[0, 0] == np.sqrt(4 * t)
    for x, Ts, ys in ((xa, T, y), (xp, 4 * T, -y)):
        assert np.isfinite(x).all() and ss.eta(Ts, x, ys) <= ss.bound(1) and ss.fwd(x, ys / Ts[0]) <= ss.bound(1)


# ----------------------------------------------------------------------------------------------------------------- 2. bits
@pytest.mark.parametrize("M", [129, 333])
def test_same_bits_twice_alone_and_swapped(M):
    a, p = _pair(M, 1e-3)
    first = _solve(a["T"], a["y"], p["T"], p["y"])
    again = _solve(a["T"], a["y"], p["T"], p["y"])
    assert all(_same(u, v) for u, v in zip(first[:4], again[:4])) and first[4].tolist() == again[4].tolist() == [0, 0]
    xa, _, La, _, info = _solve(a["T"], a["y"])
    assert info.tolist() == [0, 0] and _same(xa, first[0]) and _same(La, first[2])
    xp, xa2, Lp, La2, info = _solve(p["T"], p["y"], a["T"], a["y"])
    assert info.tolist() == [0, 0]
    assert _same(xa2, first[0]) and _same(La2, first[2]) and _same(xp, first[1]) and _same(Lp, first[3])


# -------------------------------------------------------------------------------------------------------------- 3. failure
@pytest.mark.parametrize("p,bad", [(0, -1.0), (5, -1.0), (63, -1.0), (64, -1.0), (65, -1.0), (130, -1.0), (199, -1.0), (64, np.nan)])
def test_failed_pivot_is_a_status(p, bad):
    a, ph = _pair(200, 1e-3)
    healthy = _solve(a["T"], a["y"], ph["T"], ph["y"])
    Tb = a["T"].copy()
    Tb[p, p] = bad
    if bad == bad:
        assert ss.lapack_solve(Tb, a["y"])[1] == p + 1
    xa, xp, _, Lp, info = _solve(Tb, a["y"], ph["T"], ph["y"])
    assert info.tolist() == [p + 1, 0]
    assert np.isnan(xa).all() and _same(xp, healthy[1]) and _same(Lp, healthy[3])
    # the failing system in the phi slot
    xp, xa, Lp, _, info = _solve(ph["T"], ph["y"], Tb, a["y"])
    assert info.tolist() == [0, p + 1]
    assert np.isnan(xa).all() and _same(xp, healthy[1]) and _same(Lp, healthy[3])
    # and alone
    xa, _, _, _, info = _solve(Tb, a["y"])
    assert info.tolist() == [p + 1, 0] and np.isnan(xa).all()


# ------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals():
    fused = _fused()
    n = 70
    (T, y), _ = ss.pair(n, 1e-3)
    buf = dict(Ta=_dev(T), Tp=_dev(T), ya=_dev(y), yp=_dev(y), xa=torch.zeros(n, dtype=torch.float64, device="cuda"),
               xp=torch.zeros(n, dtype=torch.float64, device="cuda"), info=torch.zeros(2, dtype=torch.int32, device="cuda"))

    def call(M, handle=fused._h, **null):
        ptr = {k: (None if k in null else v.data_ptr()) for k, v in buf.items()}
        return fused._lib.naqs_net_sr_solve(handle, M, ptr["Ta"], ptr["Tp"], ptr["ya"], ptr["yp"], ptr["xa"], ptr["xp"], ptr["info"],
                                            _stream_ptr(fused.device))

    assert call(n, handle=None) == -1
    for name in ("Ta", "ya", "xa", "info"):
        assert call(n, **{name: 1}) == -1, name
    for part in (("Tp",), ("yp",), ("xp",), ("Tp", "yp"), ("Tp", "xp"), ("yp", "xp")):
        assert call(n, **dict.fromkeys(part, 1)) == -1, part
    assert call(0) == -1 and call(-3) == -1
    torch.cuda.synchronize()
    assert torch.equal(buf["Ta"], _dev(T)) and int(buf["xa"].abs().sum()) == 0          # nothing was touched
    # 1-element buffers as in test_sr_gpu._raw_gram: the refused size never reaches them
    buf = {k: torch.zeros(2 if k == "info" else 1, dtype=v.dtype, device="cuda") for k, v in buf.items()}
    assert call(32769) == -4
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ 5. the real systems
@pytest.mark.parametrize("case", sr.CASES, ids=sr.case_id)
def test_direction_through_the_hip_solve(case):
    import test_sr_gpu as tg
    r = tg._reference(case)
    fused = r["fused"]
    M = len(r["keys"])
    kd, w, g, A, B = tg._leading(r, M)
    _, saved = fused.forward_saved(kd)
    wd = tg._dev(w)
    Ta, Tp, ya, yp = fused.sr_gram(saved, wd, tg._dev(g, torch.float32), tg.SHIFT)
    x_torch = [tg._solve(Ta, ya), tg._solve(Tp, yp)]
    xa, xp, info = fused.sr_solve(Ta, Tp, ya, yp)
    assert info.tolist() == [0, 0]
    d = fused.sr_direction(saved, wd, xa, xp)
    torch.cuda.synchronize()
    d = d.double().cpu().numpy()
    g64 = g.astype(np.float64)
    d64 = sr.direction(A, B, w, g64, tg.SHIFT)
    grad64 = A.T @ g64[:, 0] + B.T @ g64[:, 1]
    err = sr.per_tensor_err(r["w64"], d, d64)
    c2 = 4 * tg.C2_YARDSTICK[sr.case_id(case)]
    print(f"\n[sr solve direction] {sr.case_id(case)} M={M}: per-tensor error {err:.3e} (bound {c2:.2e}), d.grad64 {d @ grad64:.3e}, "
          f"fwd hip / torch: a {ss.fwd(xa.cpu().numpy(), x_torch[0].cpu().numpy()):.3e} phi {ss.fwd(xp.cpu().numpy(), x_torch[1].cpu().numpy()):.3e}")
    assert np.isfinite(d).all() and err <= c2, (case, err)
    assert d @ grad64 > 0


# ----------------------------------------------------------------------------------------------------------- 6. optimiser
def _refuse(what):
    def f(*a, **k):
        raise AssertionError(what)
    return f


def test_hip_solver_takes_the_step_without_torch_cholesky(tmp_path, capsys, monkeypatch):
    import test_sr_gpu as tg
    hil, wf = gr.sector_net("LiH", seed=111)
    opt = tg._opt(wf, tmp_path, natural_gradient=dict(tg.SR_HYPER, solver="hip"))
    before = wf.flatten_parameters().clone()
    monkeypatch.setattr(torch.linalg, "cholesky_ex", _refuse("torch.linalg.cholesky_ex in a solver='hip' step"))
    monkeypatch.setattr(torch, "cholesky_solve", _refuse("torch.cholesky_solve in a solver='hip' step"))
    opt.run(n_epochs=3, save_freq=None, save_final=False, output_freq=10)
    torch.cuda.synchronize()
    capsys.readouterr()
    after = wf.flatten_parameters()
    assert opt.sr_last["solver"] == "hip" and torch.isfinite(after).all() and not torch.equal(before, after)


def test_torch_solver_and_absent_key_never_call_sr_solve_and_agree(tmp_path, capsys, monkeypatch):
    import test_sr_gpu as tg
    res = {}
    for how, ng in (("absent", dict(tg.SR_HYPER)), ("torch", dict(tg.SR_HYPER, solver="torch"))):
        hil, wf = gr.sector_net("LiH", seed=111)
        opt = tg._opt(wf, tmp_path / how, natural_gradient=ng)
        monkeypatch.setattr(wf.fused(need_phase=True), "sr_solve", _refuse("sr_solve in a torch-solver step"))
        opt.run(n_epochs=3, save_freq=None, save_final=False, output_freq=10)
        torch.cuda.synchronize()
        assert opt.sr_last["solver"] == "torch"
        res[how] = wf.flatten_parameters().clone()
    capsys.readouterr()
    assert torch.equal(res["absent"], res["torch"])


def test_hip_solver_trains_lih_below_adam(tmp_path, capsys):
    """LiH, seed 111, 100 steps each of Adam and of the natural gradient with solver="hip" at test_sr_gpu.SR_HYPER, from the same
    initial parameters.  The energy beside the torch solve's (profiles/sr.txt: -7.774103) is printed, not asserted: 100 steps
    amplify last-bit differences of the two solvers by an amount nobody has measured."""
    import test_sr_gpu as tg
    energy = {}
    for how, kw in (("adam", {}), ("hip", dict(natural_gradient=dict(tg.SR_HYPER, solver="hip")))):
        hil, wf = gr.sector_net("LiH", seed=111)
        opt = tg._opt(wf, tmp_path / how, **kw)
        before = opt.calculate_energy(normalise_psi=True)
        opt.run(n_epochs=100, save_freq=None, save_final=False, output_freq=50)
        after = opt.calculate_energy(normalise_psi=True)
        assert all(torch.isfinite(p).all() for p in wf.model.parameters()), how
        energy[how] = (before, after)
    capsys.readouterr()
    print(f"\n[sr solve training] LiH 100 steps: Adam {energy['adam'][0]:.6f} -> {energy['adam'][1]:.6f}, natural gradient with the "
          f"HIP solve {energy['hip'][0]:.6f} -> {energy['hip'][1]:.6f} Ha (torch solve, profiles/sr.txt: -7.774103)")
    assert energy["hip"][0] == energy["adam"][0]
    assert np.isfinite(energy["hip"][1]) and energy["hip"][1] < energy["hip"][0]
    assert energy["hip"][1] < energy["adam"][1]


def test_failed_factorisation_raises_and_leaves_the_parameters(tmp_path, capsys, monkeypatch):
    import test_sr_gpu as tg
    from naqs_amd.optimizer import NaturalGradientError
    hil, wf = gr.sector_net("LiH", seed=111)
    opt = tg._opt(wf, tmp_path, natural_gradient=dict(tg.SR_HYPER, solver="hip"))
    fused = wf.fused(need_phase=True)

    def gram(saved, w, g, shift):
        M = saved[0].shape[0]
        eye = torch.eye(M, dtype=torch.float64, device="cuda")
        y = torch.ones(M, dtype=torch.float64, device="cuda")
        return -eye, eye.clone(), y, y.clone()

    monkeypatch.setattr(fused, "sr_gram", gram)
    before = wf.flatten_parameters().clone()
    with pytest.raises(NaturalGradientError, match=r"amplitude block .* leading minor 1$"):
        opt.run(n_epochs=1, save_freq=None, save_final=False, output_freq=10)
    capsys.readouterr()
    torch.cuda.synchronize()
    assert torch.equal(before, wf.flatten_parameters())
