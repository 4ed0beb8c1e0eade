"""Natural gradient with momentum (SPRING) on the MI355X: ``naqs_net_sr_jvp`` and the optimiser's step with ``momentum``, against
the float64 definitions of tests/spring_reference.py (tables and float64 Jacobians: ``test_sr_gpu._reference``).

1. JVP against float64.  ``sr_reference.CASES`` at M = 1, 63, 64, 65, 200 rows and ``sr_reference.WIDTH_CASES`` at 65 rows, a seeded
   normal v and — no cancellation — v = the float32-rounded row k = M // 2 of the block's own float64 Jacobian (u_k = |J_k|^2: scale
   and value coincide).  Measure: max_i |u_i - (J64 v)_i| / (|J64| |v|)_i.  Yardstick: the float32 PyTorch network on the CPU on
   the same measure (float32 Jacobian rows times v in float64); its worst case over all these cases and both operands is 5.84e-8
   (LiH, single phase [64, 64], amplitude width 64), C_JVP = 4 x that.  The kernels' worst case on the MI355X is printed per case
   [profiles/sr_spring.txt].
2. The job -> parameter map, tensor by tensor: v non-zero on one parameter tensor at a time, every tensor of one single-phase
   and one aggregate case, to the same bound C_JVP.  With nothing else in v, |J| |v| holds one factor alone, and the float32
   stage's d-out = [c == occ] - softmax and d-pre = W2^T d-out are cancelling sums: taken from that stage, LiH aggregate's
   amp_layers.2.layers.0.0.bias came out at 3.85e-7 (the float32 CPU network: 2.95e-7 on the same operand).  The entry
   therefore recomputes the blocks' h, d-pre and d-out in float64 and rounds them once (sr_amp_factors64_kernel).
3. Against the library's own Gram matrix at run sizes (LiF, M = 1 025 and 4 097, no CPU Jacobian): v = naqs_net_train_backward of
   the unit seed at row k is row k of the Jacobian, so u = G[:, k] to C sqrt(G_ii G_kk), C of test_sr_gpu.py; and the leading
   1 025 entries at M = 4 097 have the bits of the M = 1 025 call.
4. Determinism and refusals.
5. Off means off: ``momentum=0.0`` and no ``momentum`` take the same launches to the same bits and never call ``sr_jvp``; at
   mu = 0.9 the first step is the plain step bit for bit and the second is not.
6. One SPRING step against float64: mu = 0.9, phi_prev = the float32-rounded plain direction, per-tensor error against 4 x the
   float32-CPU pipeline's (``spring_reference.spring_direction_f32``), recorded per case in STEP_YARDSTICK; and phi . grad64 > 0.
7. Training: LiH, the whole 225-state space as the table, seed 111, 100 steps, mu in {0, 0.5, 0.9, 0.99}.
"""
import numpy as np
import pytest

import grad_reference as gr
import spring_reference as spring
import sr_reference as sr
import test_sr_gpu as tg
from naqs_amd.hamiltonian import _stream_ptr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C_JVP = 4 * 5.84e-8      # 4 x the float32-CPU network's worst |J32 v - J64 v|_i / (|J64| |v|)_i (LiH-single-a64-p64x64-sym-PARTIAL)
STEP_YARDSTICK = {       # the float32-CPU pipeline's per-tensor error of one SPRING step (spring_reference.spring_direction_f32)
    "H2-single-a16-p32-sym-PARTIAL": 2.156e-06,
    "H2-agg-a16-p32-nosym-FULL": 8.276e-08,
    "syn10_3_2-single-a64-p64x64-sym-FULL": 2.416e-05,
    "syn10_3_2-agg-a64-p32-sym-PARTIAL": 1.159e-05,
    "LiH-single-a16-p32-nosym-PARTIAL": 9.462e-06,
    "LiH-single-a64-p64x64-sym-PARTIAL": 1.524e-04,
    "LiH-agg-a16-p32-sym-FULL": 1.966e-02,
    "syn32_8_8-single-a64-p32-sym-PARTIAL": 3.266e-07,
    "syn32_8_8-single-a16-p64x64-nosym-FULL": 2.851e-07,
    "syn32_8_8-agg-a64-p32-nosym-PARTIAL": 3.184e-07,
}
MU = 0.9
_kdev, _dev = tg._kdev, tg._dev


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32)


def _jvp(fused, saved, v):
    ua, up = fused.sr_jvp(saved, torch.as_tensor(_f32(v), device="cuda"))
    torch.cuda.synchronize()
    return ua.cpu().numpy(), up.cpu().numpy()


# ------------------------------------------------------------------------------------------------------- 1. JVP against float64
def _jvp_case(fused, keys, A, B, sizes):
    """The worst error over ``sizes`` leading rows, both blocks and both operands."""
    worst = 0.0
    for M in sizes:
        _, saved = fused.forward_saved(_kdev(keys[:M]))
        k = M // 2
        v = _f32(np.random.RandomState(13).normal(size=A.shape[1])).astype(np.float64)
        ua, up = _jvp(fused, saved, v)
        ra, _ = _jvp(fused, saved, A[k])
        _, rp = _jvp(fused, saved, B[k])
        for u, J, vv in ((ua, A[:M], v), (up, B[:M], v), (ra, A[:M], _f32(A[k]).astype(np.float64)), (rp, B[:M], _f32(B[k]).astype(np.float64))):
            assert u.shape == (M,) and np.isfinite(u).all()
            err = spring.jvp_err(u, J, vv)
            worst = max(worst, err)
            assert err <= C_JVP, (M, err)
        assert ra[k] > 0 and rp[k] > 0
    return worst


@pytest.mark.parametrize("case", sr.CASES, ids=sr.case_id)
def test_jvp_against_float64(case):
    r = tg._reference(case)
    worst = _jvp_case(r["fused"], r["keys"], r["A"], r["B"], tg._rows(len(r["keys"])))
    print(f"\n[sr jvp] {sr.case_id(case)}: worst |u - J64 v| / (|J64| |v|) {worst:.3e} (bound {C_JVP:.2e})")


@pytest.mark.parametrize("case", sr.WIDTH_CASES, ids=sr.case_id)
def test_jvp_at_amplitude_widths(case):
    hil, wf = sr.make_net(case, device="cuda")
    fused = wf.fused(need_phase=True)
    assert fused is not None and fused.train_mode == "hip", case
    _, w64 = gr.f64_copy(wf)
    keys, _ = sr.table(hil, w64)
    keys = keys[:65]
    A, B = sr.jacobians(w64, sr.states_of(hil, keys))
    worst = _jvp_case(fused, keys, A, B, (65,))
    print(f"\n[sr jvp widths] {sr.case_id(case)}: worst |u - J64 v| / (|J64| |v|) {worst:.3e} (bound {C_JVP:.2e})")


# ------------------------------------------------------------------------------------------------------ 2. map, tensor by tensor
@pytest.mark.parametrize("case", [sr.CASES[5], sr.CASES[6]], ids=sr.case_id)
def test_every_parameter_tensor_meets_its_own_layer(case):
    r = tg._reference(case)
    M = 65
    A, B = r["A"][:M], r["B"][:M]
    _, saved = r["fused"].forward_saved(_kdev(r["keys"][:M]))
    v = _f32(np.random.RandomState(13).normal(size=A.shape[1])).astype(np.float64)
    names = [n for n, _ in r["w64"].model.named_parameters()]
    P = len(r["w64"].model.amp_layers)
    assert any(n.startswith("amp_layers.0.") for n in names) and any(n.startswith(f"amp_layers.{P - 1}.") for n in names)
    off = 0
    for name, p in r["w64"].model.named_parameters():
        e = np.zeros_like(v)
        e[off:off + p.numel()] = v[off:off + p.numel()]
        off += p.numel()
        ua, up = _jvp(r["fused"], saved, e)
        for u, J in ((ua, A), (up, B)):
            err = spring.jvp_err(u, J, e)
            assert err <= C_JVP, (name, err)
        # a tensor that moves a block moves it here too (pair 0's first-layer weights meet the constant-zero input: both zero)
        assert (np.abs(ua).max() > 0) == (np.abs(A @ e).max() > 0) and (np.abs(up).max() > 0) == (np.abs(B @ e).max() > 0), name
    assert off == len(v)


# ------------------------------------------------------------------------------------------- 3. the library's own Gram matrix
def test_jvp_of_a_jacobian_row_is_a_gram_column_at_run_sizes():
    hil, wf = sr.make_net(sr.LARGE_CASES[0], device="cuda")
    fused = wf.fused(need_phase=True)
    assert fused is not None and fused.train_mode == "hip"
    keys = np.sort(gr.random_keys(hil, 4097, seed=5))
    assert len(keys) == 4097
    kept = {}
    worst = 0.0
    for M in (1025, 4097):
        kd = _kdev(keys[:M])
        _, saved = fused.forward_saved(kd)
        Ga, Gp = fused.sr_gram(saved, None, None, None, uncentred=True)
        da, dp = Ga.diagonal().sqrt(), Gp.diagonal().sqrt()
        for k in (0, 64, M - 1):
            seeds = torch.zeros((M, 2), dtype=torch.float32, device="cuda")
            seeds[k] = 1.0                                  # row k of A and of B at once: disjoint parameters
            v = torch.empty(fused.n_params, dtype=torch.float32, device="cuda")
            st = fused._lib.naqs_net_train_backward(fused._h, M, kd.data_ptr(), seeds.data_ptr(), v.data_ptr(), _stream_ptr(fused.device))
            assert st == 0
            ua, up = fused.sr_jvp(saved, v)
            if M == 1025:
                kept[k] = (v, ua.clone(), up.clone())
            for u, G, d in ((ua, Ga, da), (up, Gp, dp)):
                err = float(((u - G[:, k]).abs() / (d * d[k])).max())
                worst = max(worst, err)
                assert err <= tg.C, (M, k, err)
        del Ga, Gp
    for k in (0, 64):                                       # (saved: the table of 4 097 rows) the same v, the rows both tables hold
        v, ua, up = kept[k]
        for small, large in zip((ua, up), fused.sr_jvp(saved, v)):
            assert torch.equal(small, large[:1025]), k
    print(f"\n[sr jvp] LiF M = 1025, 4097: worst |u - G[:, k]| / sqrt(G_ii G_kk) {worst:.3e} (bound {tg.C:.2e})")


# ------------------------------------------------------------------------------------------------ 4. determinism and refusals
def _raw_jvp(fused, M, kd):
    v = torch.zeros(fused.n_params, dtype=torch.float32, device="cuda")
    u = torch.zeros((2, M if 0 < M <= 1024 else 1), dtype=torch.float64, device="cuda")      # (the refused sizes never reach the buffers)
    return fused._lib.naqs_net_sr_jvp(fused._h, M, kd.data_ptr(), v.data_ptr(), u[0].data_ptr(), u[1].data_ptr(), _stream_ptr(fused.device))


@pytest.mark.parametrize("case", [sr.CASES[5], sr.CASES[6]], ids=sr.case_id)
def test_same_bits_twice_and_at_any_table_that_holds_the_row(case):
    r = tg._reference(case)
    fused = r["fused"]
    v = torch.as_tensor(_f32(np.random.RandomState(13).normal(size=r["A"].shape[1])), device="cuda")
    M = len(r["keys"])
    _, saved = fused.forward_saved(_kdev(r["keys"]))
    first, second = fused.sr_jvp(saved, v), fused.sr_jvp(saved, v)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    _, saved = fused.forward_saved(_kdev(r["keys"][:65]))
    part = fused.sr_jvp(saved, v)
    assert M > 65 and all(torch.equal(a[:65], b) for a, b in zip(first, part))


@pytest.mark.parametrize("aggregate", [False, True], ids=["single", "aggregate"])
def test_invalid_arguments_and_no_held_forward(aggregate):
    hil, wf = gr.sector_net("LiH", aggregate=aggregate, amp_hidden=16, phase_hidden=(32,))
    fused = wf.fused(need_phase=True)
    kd = _kdev(np.sort(gr.random_keys(hil, 70, seed=1)))
    assert _raw_jvp(fused, 70, kd) == -1                                          # no training forward yet
    fused.forward_saved(kd)
    assert _raw_jvp(fused, 70, kd) == 0
    assert _raw_jvp(fused, 0, kd) == -1 and _raw_jvp(fused, 32769, kd) == -4
    u = torch.zeros(70, dtype=torch.float64, device="cuda")
    v = torch.zeros(fused.n_params, dtype=torch.float32, device="cuda")
    s = _stream_ptr(fused.device)
    for args in ((None, v.data_ptr(), u.data_ptr(), u.data_ptr()), (kd.data_ptr(), None, u.data_ptr(), u.data_ptr()),
                 (kd.data_ptr(), v.data_ptr(), None, u.data_ptr()), (kd.data_ptr(), v.data_ptr(), u.data_ptr(), None)):
        assert fused._lib.naqs_net_sr_jvp(fused._h, 70, *args, s) == -1
    with pytest.raises(ValueError, match="sr_jvp"):
        fused.sr_jvp((kd, None, None), v[:-1])
    torch.cuda.synchronize()


@pytest.mark.parametrize("family", [dict(combined=True), dict(amp_layers=2), dict(aggregate=True, amp_layers=2, phase_hidden=(64, 64))],
                         ids=["combined", "amp_layers", "agg_layers"])
def test_combined_and_deep_handles_are_unsupported(family):
    args = dict(phase_hidden=(64, 64))
    args.update(family)
    hil, wf = gr.sector_net("LiH", **args)
    fused = wf.fused(need_phase=True)
    assert fused is not None
    kd = _kdev(np.sort(gr.random_keys(hil, 70, seed=1)))
    fused.forward_saved(kd)
    assert _raw_jvp(fused, 70, kd) == -4
    with pytest.raises(NotImplementedError, match="natural gradient"):
        fused.sr_jvp((kd, None, None), torch.zeros(fused.n_params, device="cuda"))


# ---------------------------------------------------------------------------------------------------------- 5. off means off
def test_no_momentum_and_zero_momentum_are_the_plain_step(tmp_path, capsys, monkeypatch):
    from naqs_amd import _lib
    lib = _lib.load_library()
    res = {}
    for how, ng in (("absent", tg.SR_HYPER), ("zero", dict(tg.SR_HYPER, momentum=0.0)), ("spring", dict(tg.SR_HYPER, momentum=MU))):
        hil, wf = gr.sector_net("LiH", seed=111)
        opt = tg._opt(wf, tmp_path / how, natural_gradient=ng)
        fused = wf.fused(need_phase=True)
        calls = []
        if how != "spring":
            def refuse(*a, **k):
                raise AssertionError("a Jacobian-vector product in a step without momentum")
            monkeypatch.setattr(fused, "sr_jvp", refuse)
        else:
            jvp = fused.sr_jvp
            monkeypatch.setattr(fused, "sr_jvp", lambda *a, **k: calls.append(1) or jvp(*a, **k))
        params, update = [], opt._natural_gradient_update

        def step(*a, _update=update, _wf=wf, _params=params):
            _update(*a)
            _params.append(_wf.flatten_parameters().clone())

        monkeypatch.setattr(opt, "_natural_gradient_update", step)
        n0 = lib.naqs_launch_count()
        opt.run(n_epochs=3, save_freq=None, save_final=False, output_freq=10)
        torch.cuda.synchronize()
        assert len(params) == 3
        res[how] = (lib.naqs_launch_count() - n0, params, len(calls), dict(opt.sr_last))
    capsys.readouterr()
    assert res["absent"][0] == res["zero"][0] and all(torch.equal(a, b) for a, b in zip(res["absent"][1], res["zero"][1]))
    assert res["zero"][3]["momentum"] == 0.0 and "jvp_norm" not in res["zero"][3]
    # mu = 0.9: the first step has no previous step and is the plain one; the later ones are not
    assert torch.equal(res["spring"][1][0], res["absent"][1][0])
    assert not torch.equal(res["spring"][1][1], res["absent"][1][1]) and not torch.equal(res["spring"][1][2], res["absent"][1][2])
    assert res["spring"][2] == 2 and res["spring"][0] > res["absent"][0]
    assert res["spring"][3]["momentum"] == MU and float(res["spring"][3]["jvp_norm"]) > 0


def test_previous_step_travels_with_the_checkpoint(tmp_path, capsys):
    """phi_prev is saved under its own key only when mu > 0, comes back on load, is cleared by ``reset_optimizer``, and a
    checkpoint without it (a plain natural-gradient run's) loads into a momentum run as "no previous step"."""
    ng = dict(tg.SR_HYPER, momentum=MU)
    hil, wf = gr.sector_net("LiH", seed=111)
    opt = tg._opt(wf, tmp_path / "spring", natural_gradient=ng)
    assert getattr(opt, "_sr_phi_prev", None) is None
    opt.run(n_epochs=2, save_freq=None, save_final=False, output_freq=10)
    prev = opt._sr_phi_prev.clone()
    assert prev.dtype == torch.float32 and prev.shape == wf.flatten_parameters().shape and float(prev.norm()) > 0
    opt.save("ck", quiet=True)
    _, wf_plain = gr.sector_net("LiH", seed=111)
    plain = tg._opt(wf_plain, tmp_path / "plain", natural_gradient=tg.SR_HYPER)
    plain.run(n_epochs=1, save_freq=None, save_final=False, output_freq=10)
    plain.save("ck", quiet=True)
    assert "natural_gradient:phi_prev" in torch.load(tmp_path / "spring" / "ck.pth", weights_only=False)
    assert "natural_gradient:phi_prev" not in torch.load(tmp_path / "plain" / "ck.pth", weights_only=False)
    _, wf2 = gr.sector_net("LiH", seed=5)
    opt2 = tg._opt(wf2, tmp_path / "spring", natural_gradient=ng)
    opt2.load("ck", quiet=True)
    assert torch.equal(opt2._sr_phi_prev, prev) and torch.equal(wf2.flatten_parameters(), wf.flatten_parameters())
    opt2.reset_optimizer()
    assert opt2._sr_phi_prev is None
    opt2._sr_phi_prev = prev
    opt2.load(str(tmp_path / "plain" / "ck.pth"), quiet=True)
    assert opt2._sr_phi_prev is None
    capsys.readouterr()


# -------------------------------------------------------------------------------------------- 6. one SPRING step against float64
# (every case with torch's solves; the library's solver on one single-phase and one aggregate case)
@pytest.mark.parametrize("case,solver", [(c, "torch") for c in sr.CASES] + [(sr.CASES[5], "hip"), (sr.CASES[6], "hip")],
                         ids=lambda a: a if isinstance(a, str) else sr.case_id(a))
def test_spring_step_against_float64(case, solver):
    from naqs_amd.optimizer import PartialSamplingOptimizer
    r = tg._reference(case)
    fused = r["fused"]
    M = len(r["keys"])
    kd, w, g, A, B = tg._leading(r, M)
    g64 = g.astype(np.float64)
    prev = _f32(sr.direction(A, B, w, g64, tg.SHIFT))
    phi64 = spring.spring_direction(A, B, w, g64, tg.SHIFT, MU, prev.astype(np.float64))
    grad64 = A.T @ g64[:, 0] + B.T @ g64[:, 1]

    class Wf:                                               # the step goes to a scratch vector, not to the shared network
        p = torch.zeros(fused.n_params, dtype=torch.float32, device="cuda")

        def flatten_parameters(self):
            return self.p

    opt = object.__new__(PartialSamplingOptimizer)
    opt.natural_gradient, opt.wavefunction = dict(diag_shift=tg.SHIFT, lr=1.0, momentum=MU, solver=solver), Wf()
    opt._sr_phi_prev = torch.as_tensor(prev, device="cuda")
    _, saved = fused.forward_saved(kd)
    opt._natural_gradient_update(fused, saved, _dev(w), _dev(g, torch.float32))
    torch.cuda.synchronize()
    phi = opt._sr_phi_prev.double().cpu().numpy()
    assert np.array_equal(-Wf.p.double().cpu().numpy(), phi) and opt.sr_last["solver"] == solver
    err = sr.per_tensor_err(r["w64"], phi, phi64)
    c2 = 4 * STEP_YARDSTICK[sr.case_id(case)]
    print(f"\n[sr spring step] {sr.case_id(case)} M={M} mu={MU} {solver}: per-tensor error {err:.3e} (bound {c2:.2e}), "
          f"phi.grad64 {phi @ grad64:.3e}, |X phi_prev| {float(opt.sr_last['jvp_norm']):.3e}")
    assert np.isfinite(phi).all() and err <= c2, (case, err)
    assert phi @ grad64 > 0


# --------------------------------------------------------------------------------------------------------------- 7. training
GRID = (0.0, 0.5, 0.9, 0.99)
_TRAIN = {}


def _train(tmp_path, mu, solver=None, plain=False):
    key = (mu, solver, plain)
    if key not in _TRAIN:
        ng = dict(tg.SR_HYPER) if plain else dict(tg.SR_HYPER, momentum=mu)
        if solver is not None:
            ng["solver"] = solver
        hil, wf = gr.sector_net("LiH", seed=111)
        opt = tg._opt(wf, tmp_path / f"mu{mu}_{solver}_{plain}", natural_gradient=ng)
        before = opt.calculate_energy(normalise_psi=True)
        opt.run(n_epochs=100, save_freq=None, save_final=False, output_freq=50)
        after = opt.calculate_energy(normalise_psi=True)
        finite = all(bool(torch.isfinite(p).all()) for p in wf.model.parameters())
        _TRAIN[key] = (before, after, finite)
    return _TRAIN[key]


@pytest.mark.parametrize("mu,solver", [(mu, None) for mu in GRID] + [(MU, "hip")], ids=lambda a: "torch" if a is None else str(a))
def test_spring_trains_lih(tmp_path, capsys, mu, solver):
    """LiH, the set-up of test_sr_gpu.test_natural_gradient_trains_lih_below_adam (10^7 samples per step: the table is the whole
    225-state space; seed 111; 100 steps at diag_shift 1e-3, lr 0.1) over mu in {0, 0.5, 0.9, 0.99}, and the library's solver at
    mu = 0.9.  Energies and parameters stay finite, the energy ends below its start, and mu = 0 is the plain run exactly."""
    plain = _train(tmp_path, 0.0, plain=True)
    before, after, finite = _train(tmp_path, mu, solver)
    capsys.readouterr()
    print(f"\n[sr spring training] LiH 100 steps, mu={mu:g} ({solver or 'torch'}): {before:.6f} -> {after:.6f} Ha; plain minSR -> {plain[1]:.6f} Ha")
    assert before == plain[0]
    assert finite and np.isfinite(after) and after < before, (before, after)
    if mu == 0.0:
        assert after == plain[1]
    # observed on the MI355X (bit-reproducible runs; profiles/sr_spring.txt): plain -7.774103, mu = 0.5 -7.775198, mu = 0.9 -7.774393
    # with either solver — below plain minSR; mu = 0.99 ends at -7.771214, above it, and is not asserted
    if mu in (0.5, 0.9):
        assert after < plain[1], (mu, after, plain[1])
