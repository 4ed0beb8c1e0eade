"""Natural-gradient training (minSR) on the MI355X: ``naqs_net_sr_gram`` / ``naqs_net_sr_direction`` against the float64
definitions (tests/sr_reference.py: Jacobian rows from torch.autograd on a float64 CPU copy of the network).

1. Gram against float64.  ``sr_reference.CASES`` (both families, amplitude widths 16 / 64, phase [32] / [64, 64], with and without
   the amplitude symmetry, PARTIAL / FULL masking, sectors of 2, 5, 6 and 16 pairs) at M = 1, 63, 64, 65, 200 rows (fewer where the
   sector is smaller).  |G - G64|_ij <= C sqrt(G64_ii G64_jj) for the uncentred Gram matrices, then T + lambda I and y against
   their definitions to the same bound.  The yardstick is the float32 PyTorch network on the CPU on the same quantity (float32
   Jacobian rows, products in float64): its worst case over the cases is 1.70e-7 (H2, aggregate, amplitude block), C = 4 x that.
   The kernels' worst case on the MI355X: 1.11e-7 (G), 1.22e-7 (T), y exact  [profiles/sr.txt].
2. Direction against float64 at diag_shift = 1e-2: per parameter tensor max |d - d64| <= C2 max |d64|.  The yardstick is the
   float32-CPU pipeline (sr_reference.direction_f32: float32 Jacobian rows, the systems and solves in float64, float32 seeds, the
   float32 autograd backward for X^T x), C2 = 4 x its figure, recorded per case in C2_YARDSTICK.  Per case because the figure is
   set by cancellation in the float32 backward (x is large along the near-null directions of X, X^T x is not) and spans five
   decades: 1.4e-7 (H2, aggregate) to 2.0e-2 (LiH, aggregate, FULL: a tensor whose direction is 1e-6 of the terms summed); one
   worst-case constant would check nothing elsewhere.  The kernels land on the yardstick in every case (0.6 to 1.4 x;
   profiles/sr.txt).  A first yardstick without the float32 backward (X^T x in float64: 2.05e-5 at worst) is not what any
   float32 pipeline computes; against 4 x that, LiH single [64, 64] (1.6e-4) and LiH aggregate (1.4e-2) miss.  And d . grad64 > 0.
3. Determinism: the same bits twice; seeds e_k / sqrt(w_k) reproduce naqs_net_train_backward of the equivalent g bit for bit.
4. Refusals, and a plain optimiser's step unchanged.
5. Training: LiH, the whole 225-state space as the table, seed 111, 100 steps.
"""
import ctypes
import os

import numpy as np
import pytest

import grad_reference as gr
import sr_reference as sr
from conftest import GOLDEN
from naqs_amd.hamiltonian import _stream_ptr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C = 4 * 1.70e-7          # 4 x the float32-CPU network's worst |G32 - G64|_ij / sqrt(G64_ii G64_jj)
C2_YARDSTICK = {         # the float32-CPU pipeline's per-tensor direction error (sr_reference.direction_f32), per case
    "H2-single-a16-p32-sym-PARTIAL": 1.717e-06,
    "H2-agg-a16-p32-nosym-FULL": 1.359e-07,
    "syn10_3_2-single-a64-p64x64-sym-FULL": 2.896e-05,
    "syn10_3_2-agg-a64-p32-sym-PARTIAL": 1.499e-05,
    "LiH-single-a16-p32-nosym-PARTIAL": 1.463e-05,
    "LiH-single-a64-p64x64-sym-PARTIAL": 1.434e-04,
    "LiH-agg-a16-p32-sym-FULL": 1.982e-02,
    "syn32_8_8-single-a64-p32-sym-PARTIAL": 2.570e-06,
    "syn32_8_8-single-a16-p64x64-nosym-FULL": 1.555e-06,
    "syn32_8_8-agg-a64-p32-nosym-PARTIAL": 2.925e-06,
}
SHIFT = 1e-2
SR_HYPER = dict(diag_shift=1e-3, lr=0.1)       # test 5's grid point (profiles/sr.txt)

_REF = {}


def _reference(case):
    """Per case, computed once and left unchanged: the network on the GPU, its float64 copy, a kink-free key table with
    weights and seeds, and the float64 Jacobians of the table."""
    if case not in _REF:
        hil, wf = sr.make_net(case, device="cuda")
        fused = wf.fused(need_phase=True)
        assert fused is not None and fused.train_mode == "hip", case
        _, w64 = gr.f64_copy(wf)
        keys, w = sr.table(hil, w64)
        A, B = sr.jacobians(w64, sr.states_of(hil, keys))
        rs = np.random.RandomState(7)
        e = rs.normal(-7.0, 1.0, len(keys)) + 1j * rs.normal(0.0, 0.3, len(keys))
        _REF[case] = dict(hil=hil, wf=wf, w64=w64, fused=fused, keys=keys, w=w, A=A, B=B, e=e)
    return _REF[case]


def _kdev(keys):
    return torch.as_tensor(np.asarray(keys).astype(np.int64), device="cuda")


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _rows(n):
    return sorted({min(m, n) for m in sr.ROWS})


def _leading(r, M):
    """The first M rows of a case's table: keys, weights renormalised to sum 1, float32 seeds of the VMC loss, Jacobians."""
    w = r["w"][:M] / r["w"][:M].sum()
    g = gr.loss_grad_f64(r["e"][:M], w).astype(np.float32)
    return _kdev(r["keys"][:M]), w, g, r["A"][:M], r["B"][:M]


# ------------------------------------------------------------------------------------------------------------------ 1. Gram
@pytest.mark.parametrize("case", sr.CASES, ids=sr.case_id)
def test_gram_against_float64(case):
    r = _reference(case)
    fused = r["fused"]
    worst_g = worst_t = worst_y = 0.0
    for M in _rows(len(r["keys"])):
        kd, w, g, A, B = _leading(r, M)
        _, saved = fused.forward_saved(kd)
        Ga, Gp = fused.sr_gram(saved, None, None, None, uncentred=True)
        torch.cuda.synchronize()
        Ga, Gp = Ga.cpu().numpy(), Gp.cpu().numpy()
        for G, J in ((Ga, A), (Gp, B)):
            assert np.array_equal(G, G.T), (case, M)
            err = sr.gram_err(G, J @ J.T)
            worst_g = max(worst_g, err)
            assert err <= C, (case, M, err)
        if M == 1:
            continue                                  # (one sample: T = 0 and lambda = 0 by definition — nothing to compare)
        Ta, Tp, ya, yp = fused.sr_gram(saved, _dev(w), _dev(g, torch.float32), SHIFT)
        torch.cuda.synchronize()
        for T, y, J, col in ((Ta, ya, A, 0), (Tp, yp, B, 1)):
            T64, y64, _ = sr.system(J, w, g[:, col], SHIFT)
            err_t = sr.gram_err(T.cpu().numpy(), T64)
            err_y = float(np.abs(y.cpu().numpy() - y64).max() / max(np.abs(y64).max(), 1e-300))
            worst_t, worst_y = max(worst_t, err_t), max(worst_y, err_y)
            assert err_t <= C and err_y <= C, (case, M, err_t, err_y)
    print(f"\n[sr gram] {sr.case_id(case)}: worst |G - G64| {worst_g:.3e}, |T - T64| {worst_t:.3e}, |y - y64| {worst_y:.3e} (bound {C:.2e})")


# ------------------------------------------------------------------------------------------------------------- 2. direction
def _solve(T, y):
    L, info = torch.linalg.cholesky_ex(T)
    assert int(info.item()) == 0
    return torch.cholesky_solve(y.unsqueeze(1), L).squeeze(1)


def _direction(fused, kd, w, g):
    _, saved = fused.forward_saved(kd)
    wd = _dev(w)
    Ta, Tp, ya, yp = fused.sr_gram(saved, wd, _dev(g, torch.float32), SHIFT)
    return fused.sr_direction(saved, wd, _solve(Ta, ya), _solve(Tp, yp)), (Ta, Tp, ya, yp)


@pytest.mark.parametrize("case", sr.CASES, ids=sr.case_id)
def test_direction_against_float64(case):
    r = _reference(case)
    M = len(r["keys"])
    kd, w, g, A, B = _leading(r, M)
    d, _ = _direction(r["fused"], kd, w, g)
    torch.cuda.synchronize()
    d = d.double().cpu().numpy()
    g64 = g.astype(np.float64)
    d64 = sr.direction(A, B, w, g64, SHIFT)
    grad64 = A.T @ g64[:, 0] + B.T @ g64[:, 1]
    err = sr.per_tensor_err(r["w64"], d, d64)
    c2 = 4 * C2_YARDSTICK[sr.case_id(case)]
    print(f"\n[sr direction] {sr.case_id(case)} M={M}: per-tensor error {err:.3e} (bound {c2:.2e}), d.grad64 {d @ grad64:.3e}")
    assert np.isfinite(d).all() and err <= c2, (case, err)
    assert d @ grad64 > 0


# ----------------------------------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("case", [sr.CASES[5], sr.CASES[6]], ids=sr.case_id)
def test_same_bits_twice_and_unit_seeds_are_the_backward_pass(case):
    r = _reference(case)
    fused = r["fused"]
    M = len(r["keys"])
    kd, w, g, _, _ = _leading(r, M)
    d1, sys1 = _direction(fused, kd, w, g)
    d2, sys2 = _direction(fused, kd, w, g)
    assert all(torch.equal(a, b) for a, b in zip(sys1, sys2)) and torch.equal(d1, d2)
    # x = alpha e_k / sqrt(w_k): one non-zero term in the seeds' sums, so the float64 formula below has the kernel's roundings
    wd = _dev(w)
    _, saved = fused.forward_saved(kd)
    for k, alpha in ((0, 1.0), (M // 2, -0.37), (M - 1, 2.5)):
        xa = torch.zeros(M, dtype=torch.float64, device="cuda")
        xp = torch.zeros(M, dtype=torch.float64, device="cuda")
        xa[k] = alpha / wd[k].sqrt()
        xp[(k + 1) % M] = -alpha / wd[(k + 1) % M].sqrt()
        got = fused.sr_direction(saved, wd, xa, xp)
        sq = wd.sqrt()
        seeds = torch.stack([sq * xa - wd * (sq * xa).sum(), sq * xp - wd * (sq * xp).sum()], -1).float().contiguous()
        want = torch.empty_like(got)
        st = fused._lib.naqs_net_train_backward(fused._h, M, kd.data_ptr(), seeds.data_ptr(), want.data_ptr(), _stream_ptr(fused.device))
        assert st == 0
        torch.cuda.synchronize()
        assert torch.equal(got, want), (case, k)


# -------------------------------------------------------------------------------------------------------------- 4. refusals
def _raw_gram(fused, M, kd, shift):
    w = torch.full((max(M, 1),), 1.0 / max(M, 1), dtype=torch.float64, device="cuda")
    g = torch.zeros((max(M, 1), 2), dtype=torch.float32, device="cuda")
    n = M if 0 < M <= 1024 else 1                 # (the refused sizes never reach the buffers)
    T = torch.zeros((2, n, n), dtype=torch.float64, device="cuda")
    y = torch.zeros((2, n), dtype=torch.float64, device="cuda")
    return fused._lib.naqs_net_sr_gram(fused._h, M, kd.data_ptr(), w.data_ptr(), g.data_ptr(), ctypes.c_double(shift), T[0].data_ptr(),
                                       T[1].data_ptr(), y[0].data_ptr(), y[1].data_ptr(), _stream_ptr(fused.device))


def _raw_direction(fused, M, kd):
    w = torch.full((max(M, 1),), 1.0 / max(M, 1), dtype=torch.float64, device="cuda")
    x = torch.zeros((2, max(M, 1)), dtype=torch.float64, device="cuda")
    out = torch.zeros(fused.n_params, dtype=torch.float32, device="cuda")
    return fused._lib.naqs_net_sr_direction(fused._h, M, kd.data_ptr(), w.data_ptr(), x[0].data_ptr(), x[1].data_ptr(), out.data_ptr(),
                                            _stream_ptr(fused.device))


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
    assert _raw_gram(fused, 70, kd, 1e-3) == -4 and _raw_direction(fused, 70, kd) == -4
    with pytest.raises(NotImplementedError, match="natural gradient"):
        fused.sr_gram((kd, None, None), None, None, 1e-3)


@pytest.mark.parametrize("aggregate", [False, True], ids=["single", "aggregate"])
def test_invalid_arguments_and_no_held_forward(aggregate):
    hil, wf = gr.sector_net("LiH", aggregate=aggregate, amp_hidden=16, phase_hidden=(32,))
    fused = wf.fused(need_phase=True)
    kd = _kdev(np.sort(gr.random_keys(hil, 70, seed=1)))
    assert _raw_gram(fused, 70, kd, 1e-3) == -1 and _raw_direction(fused, 70, kd) == -1          # no training forward yet
    fused.forward_saved(kd)
    assert _raw_gram(fused, 70, kd, 1e-3) == 0 and _raw_direction(fused, 70, kd) == 0
    assert _raw_gram(fused, 70, kd, 0.0) == -1 and _raw_gram(fused, 70, kd, -1e-3) == -1 and _raw_gram(fused, 70, kd, float("nan")) == -1
    assert _raw_gram(fused, 0, kd, 1e-3) == -1 and _raw_direction(fused, 0, kd) == -1
    assert _raw_gram(fused, 32769, kd, 1e-3) == -4
    torch.cuda.synchronize()


def _opt(wf, tmp, **kw):
    from naqs_amd import packing
    from naqs_amd.optimizer import PartialSamplingOptimizer
    from test_optimizer import ADAM
    ham = packing.load_packed(os.path.join(GOLDEN, "ham_LiH.npz"))
    args = dict(n_samples=int(1e7), n_samples_max=1e12, n_unq_samples_min=10, n_unq_samples_max=1e5, log_exact_energy=False,
                wavefunction=wf, qubit_hamiltonian=ham, pre_compute_H=False, n_electrons=4, n_alpha_electrons=2,
                n_beta_electrons=2, normalise_psi=True, grad_clip_factor=None, optimizer=torch.optim.Adam,
                optimizer_args=[dict(a) for a in ADAM], save_loc=str(tmp), pauli_hamiltonian_dtype=np.float64, seed=111)
    args.update(kw)
    return PartialSamplingOptimizer(**args)


def test_plain_optimiser_takes_the_launches_it_took(tmp_path, capsys, monkeypatch):
    """Without ``natural_gradient`` nothing changes: the one-call step is still taken, three steps launch the same kernels the
    same number of times whether the argument is absent or None, none of them is the natural gradient's, and the parameters
    agree bit for bit; with the argument the step is the call-by-call one and launches more."""
    from naqs_amd import _lib
    lib = _lib.load_library()
    res = {}
    for how, kw in (("absent", {}), ("none", dict(natural_gradient=None)), ("sr", dict(natural_gradient=SR_HYPER))):
        hil, wf = gr.sector_net("LiH", seed=111)
        opt = _opt(wf, tmp_path / how, **kw)
        fused = wf.fused(need_phase=True)
        assert (opt._can_onecall(), opt._can_prefuse()) == ((False, False) if how == "sr" else (True, True))
        if how != "sr":
            def refuse(*a, **k):
                raise AssertionError("a natural-gradient call in a plain step")
            monkeypatch.setattr(fused, "sr_gram", refuse)
            monkeypatch.setattr(fused, "sr_direction", refuse)
        n0 = lib.naqs_launch_count()
        opt.run(n_epochs=3, save_freq=None, save_final=False, output_freq=10)
        torch.cuda.synchronize()
        res[how] = (lib.naqs_launch_count() - n0, fused.last_kernel(), wf.flatten_parameters().clone())
    capsys.readouterr()
    assert res["absent"][0] == res["none"][0] and res["absent"][1] == res["none"][1] and torch.equal(res["absent"][2], res["none"][2])
    assert "sr_" not in res["absent"][1]
    assert res["sr"][0] > res["absent"][0] and not torch.equal(res["sr"][2], res["absent"][2])


# --------------------------------------------------------------------------------------------------------------- 5. training
def test_natural_gradient_trains_lih_below_adam(tmp_path, capsys):
    """LiH, the published network, 10^7 samples per step (the table is the whole 225-state space), seed 111: 100 natural-gradient
    steps at diag_shift 1e-3, lr 0.1 (the grid {1e-4, 1e-3} x {0.05, 0.1, 0.2} is in profiles/sr.txt) against 100 Adam steps
    with the reference's hyper-parameters from the same initial parameters."""
    energy = {}
    for how, kw in (("adam", {}), ("sr", dict(natural_gradient=SR_HYPER))):
        hil, wf = gr.sector_net("LiH", seed=111)
        opt = _opt(wf, tmp_path / how, **kw)
        before = opt.calculate_energy(normalise_psi=True)
        opt.run(n_epochs=100, save_freq=None, save_final=False, output_freq=50)
        after = opt.calculate_energy(normalise_psi=True)
        assert all(torch.isfinite(p).all() for p in wf.model.parameters()), how
        energy[how] = (before, after)
    capsys.readouterr()
    print(f"\n[sr training] LiH 100 steps: Adam {energy['adam'][0]:.6f} -> {energy['adam'][1]:.6f}, "
          f"natural gradient {energy['sr'][0]:.6f} -> {energy['sr'][1]:.6f} Ha")
    assert energy["sr"][0] == energy["adam"][0]
    assert np.isfinite(energy["sr"][1]) and energy["sr"][1] < energy["sr"][0]
    assert energy["sr"][1] < energy["adam"][1]
