"""The natural-gradient kernels (``naqs_net_sr_gram`` / ``_uncentred``, ``naqs_net_sr_jvp``, ``naqs_net_sr_direction`` and the
SPRING step on top) against float64 at every phase shape, symmetry and qubit ordering the handle accepts.  test_sr_gpu.py,
test_sr_momentum_gpu.py and test_sr_scale_gpu.py run them at phase [32] and [64, 64], ordering -1, no -phase_sym; here
(``sr_reference.SHAPE_CASES`` / ``SYM_CASES`` / ``ORDER_CASES``, each shape named for the branch it reaches):

* widths that are no multiple of 32 (sr_gram_kernel reads pad32(N) columns of rows whose leading dimension is pad64(N): the padding
  columns of the training scratch are multiplied and must be zero), multiples of 32 that are no multiple of 64, [496, 496] and the
  published [512, 512] (17 (layer, 64 columns) items: sr_jvp_kernel's deal over at most 16 workgroups wraps), [512] * 3 (25
  items), depth 8 (9 jobs); H2 (2 phase inputs) and syn32_8_8 (30, bit 31 of the keys); amplitude width 64 at [512, 512];
* -phase_sym in both families (sr_amp_factors64_kernel's raw ? d.phase_sym : d.sym arm), on LiH and the open-shell syn10_3_2;
* qubit orderings +1 and a seeded pair permutation, bit for bit against the -1 handle on relabelled keys.

1. Gram: G_a, G_phi symmetric and within C_SHAPES sqrt(G64_ii G64_jj) of J64 J64^T at M = 1, 65, 130; T + lambda I and y at
   diag_shift 1e-2 against ``sr_reference.system`` to the same bound.
2. JVP at M = 65, 130: test_sr_momentum_gpu._jvp_case's two operands, ``spring_reference.jvp_err`` <= C_JVP_SHAPES.
3. The job -> parameter map, tensor by tensor, at [16] * 8, [100, 200], one single-MLP and one aggregate -phase_sym case.
4. Direction at the whole table: per-tensor error <= 4 x DIRECTION_F32[case], and d . grad64 > 0.
5. Orderings bit for bit, one SPRING step (mu = 0.9) through the optimiser among them.
6. The padding columns are zero by construction, not by a fresh allocation: [48] after [512, 512] ran on the device, again on a
   new handle after both were destroyed, and after a training backward with random seeds on the same handle.
7. Determinism.

The bounds are computed by tests/test_sr_shapes.py (no GPU), which recomputes every figure below and fails when one is stale:
the float32 PyTorch network on the CPU against its float64 copy, per case.  C_SHAPES = max(test_sr_gpu.C, 4 x the worst GRAM_F32),
C_JVP_SHAPES = max(test_sr_momentum_gpu.C_JVP, 4 x the worst JVP_F32).  profiles/sr_shapes.txt holds the kernels' figures on the
MI355X beside them.
"""
import numpy as np
import pytest

import grad_reference as gr
import spring_reference as spring
import sr_reference as sr
import test_sr_gpu as tg
import test_sr_momentum_gpu as tm
from naqs_amd.hamiltonian import _stream_ptr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# The float32 CPU network's figures per case, as tests/test_sr_shapes.py computes them.
GRAM_F32 = {
    "LiH-single-a16-p1-nopsym-PARTIAL": 7.963e-08,
    "LiH-single-a16-p5-nopsym-PARTIAL": 7.963e-08,
    "LiH-single-a16-p33-nopsym-PARTIAL": 8.738e-08,
    "LiH-single-a16-p48-nopsym-PARTIAL": 8.652e-08,
    "LiH-single-a16-p17x17-nopsym-PARTIAL": 1.159e-07,
    "LiH-single-a16-p100x200-nopsym-PARTIAL": 7.963e-08,
    "LiH-single-a16-p96x96-nopsym-PARTIAL": 9.585e-08,
    "LiH-single-a16-p160x32-nopsym-PARTIAL": 9.849e-08,
    "LiH-single-a16-p496x496-nopsym-PARTIAL": 7.963e-08,
    "LiH-single-a16-p512x512-nopsym-PARTIAL": 7.963e-08,
    "LiH-single-a16-p512_x3-nopsym-PARTIAL": 1.258e-07,
    "LiH-single-a16-p16_x8-nopsym-PARTIAL": 7.963e-08,
    "LiH-single-a16-p64_x8-nopsym-PARTIAL": 6.534e-08,
    "H2-single-a16-p48-nopsym-PARTIAL": 3.609e-08,
    "H2-single-a16-p512x512-nopsym-PARTIAL": 3.488e-08,
    "syn32_8_8-single-a16-p48-nopsym-PARTIAL": 8.513e-08,
    "syn32_8_8-single-a16-p512x512-nopsym-PARTIAL": 6.922e-08,
    "LiH-single-a64-p512x512-nopsym-PARTIAL": 8.169e-08,
    "LiH-single-a16-p16x16-psym-PARTIAL": 1.034e-07,
    "LiH-single-a16-p48-psym-PARTIAL": 8.652e-08,
    "LiH-single-a16-p112-psym-PARTIAL": 7.963e-08,
    "LiH-single-a16-p512x512-psym-PARTIAL": 7.963e-08,
    "syn10_3_2-single-a16-p48-psym-PARTIAL": 1.018e-07,
    "LiH-agg-a16-p32-psym-PARTIAL": 6.827e-08,
    "syn10_3_2-agg-a16-p32-psym-FULL": 1.061e-07,
    "LiH-agg-a64-p48-psym-FULL": 8.741e-08,
    "syn10_3_2-agg-a64-p48-psym-PARTIAL": 9.885e-08,
}
JVP_F32 = {
    "LiH-single-a16-p1-nopsym-PARTIAL": 3.183e-08,
    "LiH-single-a16-p5-nopsym-PARTIAL": 3.745e-08,
    "LiH-single-a16-p33-nopsym-PARTIAL": 6.154e-08,
    "LiH-single-a16-p48-nopsym-PARTIAL": 3.720e-08,
    "LiH-single-a16-p17x17-nopsym-PARTIAL": 3.901e-08,
    "LiH-single-a16-p100x200-nopsym-PARTIAL": 3.501e-08,
    "LiH-single-a16-p96x96-nopsym-PARTIAL": 5.340e-08,
    "LiH-single-a16-p160x32-nopsym-PARTIAL": 8.633e-08,
    "LiH-single-a16-p496x496-nopsym-PARTIAL": 3.555e-08,
    "LiH-single-a16-p512x512-nopsym-PARTIAL": 3.819e-08,
    "LiH-single-a16-p512_x3-nopsym-PARTIAL": 4.558e-08,
    "LiH-single-a16-p16_x8-nopsym-PARTIAL": 3.089e-08,
    "LiH-single-a16-p64_x8-nopsym-PARTIAL": 3.183e-08,
    "H2-single-a16-p48-nopsym-PARTIAL": 1.669e-08,
    "H2-single-a16-p512x512-nopsym-PARTIAL": 1.669e-08,
    "syn32_8_8-single-a16-p48-nopsym-PARTIAL": 6.747e-08,
    "syn32_8_8-single-a16-p512x512-nopsym-PARTIAL": 5.110e-08,
    "LiH-single-a64-p512x512-nopsym-PARTIAL": 4.603e-08,
    "LiH-single-a16-p16x16-psym-PARTIAL": 3.183e-08,
    "LiH-single-a16-p48-psym-PARTIAL": 3.720e-08,
    "LiH-single-a16-p112-psym-PARTIAL": 3.974e-08,
    "LiH-single-a16-p512x512-psym-PARTIAL": 3.183e-08,
    "syn10_3_2-single-a16-p48-psym-PARTIAL": 5.236e-08,
    "LiH-agg-a16-p32-psym-PARTIAL": 4.458e-08,
    "syn10_3_2-agg-a16-p32-psym-FULL": 6.004e-08,
    "LiH-agg-a64-p48-psym-FULL": 3.998e-08,
    "syn10_3_2-agg-a64-p48-psym-PARTIAL": 5.277e-08,
}
DIRECTION_F32 = {
    "LiH-single-a16-p48-nopsym-PARTIAL": 2.592e-05,
    "LiH-single-a16-p100x200-nopsym-PARTIAL": 7.906e-05,
    "LiH-single-a16-p512x512-nopsym-PARTIAL": 4.206e-04,
    "LiH-single-a16-p16_x8-nopsym-PARTIAL": 6.069e-04,
    "LiH-single-a64-p512x512-nopsym-PARTIAL": 6.512e-05,
    "LiH-single-a16-p16x16-psym-PARTIAL": 7.906e-05,
    "LiH-single-a16-p48-psym-PARTIAL": 5.702e-05,
    "LiH-single-a16-p112-psym-PARTIAL": 7.906e-05,
    "LiH-single-a16-p512x512-psym-PARTIAL": 2.067e-04,
    "syn10_3_2-single-a16-p48-psym-PARTIAL": 4.462e-05,
    "LiH-agg-a16-p32-psym-PARTIAL": 1.221e-04,
    "syn10_3_2-agg-a16-p32-psym-FULL": 9.440e-05,
    "LiH-agg-a64-p48-psym-FULL": 1.597e-04,
    "syn10_3_2-agg-a64-p48-psym-PARTIAL": 6.797e-05,
}
C_SHAPES = max(tg.C, 4 * max(GRAM_F32.values()))
C_JVP_SHAPES = max(tm.C_JVP, 4 * max(JVP_F32.values()))
SHIFT = tg.SHIFT
MU = 0.9
ALL_CASES = sr.SHAPE_CASES + sr.SYM_CASES
_LIH = {c[3]: c for c in sr.SHAPE_CASES if c[0] == "LiH" and c[2] == 16}
DIRECTION_CASES = [_LIH[(48,)], _LIH[(100, 200)], _LIH[(512, 512)], ("LiH", False, 64, (512, 512), False, "PARTIAL"), _LIH[(16,) * 8]] + \
    sr.SYM_CASES
MAP_CASES = [_LIH[(16,) * 8], _LIH[(100, 200)], sr.SYM_CASES[1], sr.SYM_CASES[5]]
DETERMINISM_CASES = [_LIH[(512, 512)], sr.SYM_CASES[7]]
_kdev, _dev, _f32, _jvp = tg._kdev, tg._dev, tm._f32, tm._jvp

_REF = {}


def _handle(wf, what):
    fused = wf.fused(need_phase=True)
    assert fused is not None and fused.train_mode == "hip", what
    return fused


def _reference(case):
    """Per case, computed once and left unchanged: the network on the GPU, its float64 copy, a kink-free key table of at most 130
    rows with weights and local energies, and the float64 Jacobian of the table (A + B and B's columns: ``_jac``)."""
    if case not in _REF:
        hil, wf = sr.shape_net(case, device="cuda")
        fused = _handle(wf, case)
        _, w64 = gr.f64_copy(wf)
        keys, w = sr.table(hil, w64, rows=sr.SHAPE_TABLE)
        assert sr.rows_wanted(hil) <= len(keys) <= sr.SHAPE_TABLE, (case, len(keys))
        J, pcols = sr.split_jacobian(*sr.jacobians(w64, sr.states_of(hil, keys)))
        rs = np.random.RandomState(7)
        e = rs.normal(-7.0, 1.0, len(keys)) + 1j * rs.normal(0.0, 0.3, len(keys))
        _REF[case] = dict(hil=hil, wf=wf, w64=w64, fused=fused, keys=keys, w=w, J=J, pcols=pcols, e=e)
    return _REF[case]


def _jac(r, M):
    """(A, B) of the leading M rows."""
    J = r["J"][:M]
    return np.where(r["pcols"], 0.0, J), np.where(r["pcols"], J, 0.0)


def _leading(r, M):
    w = r["w"][:M] / r["w"][:M].sum()
    g = gr.loss_grad_f64(r["e"][:M], w).astype(np.float32)
    return _kdev(r["keys"][:M]), w, g


# ------------------------------------------------------------------------------------------------------------------ 1. Gram
@pytest.mark.parametrize("case", ALL_CASES, ids=sr.shape_id)
def test_gram_against_float64(case):
    r = _reference(case)
    fused = r["fused"]
    worst_g = worst_t = worst_y = 0.0
    for M in sr.shape_rows(len(r["keys"])):
        kd, w, g = _leading(r, M)
        A, B = _jac(r, M)
        _, saved = fused.forward_saved(kd)
        Ga, Gp = fused.sr_gram(saved, None, None, None, uncentred=True)
        torch.cuda.synchronize()
        for G, J in ((Ga.cpu().numpy(), A), (Gp.cpu().numpy(), B)):
            assert np.array_equal(G, G.T), (case, M)
            err = sr.gram_err(G, J @ J.T)
            worst_g = max(worst_g, err)
            assert err <= C_SHAPES, (case, M, err)
        if M == 1:
            continue                                  # (one sample: T = 0 and lambda = 0 by definition — nothing to compare)
        Ta, Tp, ya, yp = fused.sr_gram(saved, _dev(w), _dev(g, torch.float32), SHIFT)
        torch.cuda.synchronize()
        for T, y, J, col in ((Ta, ya, A, 0), (Tp, yp, B, 1)):
            T64, y64, _ = sr.system(J, w, g[:, col], SHIFT)
            err_t = sr.gram_err(T.cpu().numpy(), T64)       # (both triangles: T is symmetric to rounding, not bit for bit)
            err_y = float(np.abs(y.cpu().numpy() - y64).max() / max(np.abs(y64).max(), 1e-300))
            worst_t, worst_y = max(worst_t, err_t), max(worst_y, err_y)
            assert err_t <= C_SHAPES and err_y <= C_SHAPES, (case, M, err_t, err_y)
    cid = sr.shape_id(case)
    print(f"\n[sr shapes gram] {cid}: worst |G - G64| {worst_g:.3e}, |T - T64| {worst_t:.3e}, |y - y64| {worst_y:.3e} "
          f"(float32 CPU {GRAM_F32[cid]:.3e}, bound {C_SHAPES:.2e})")


# ------------------------------------------------------------------------------------------------------------------- 2. JVP
@pytest.mark.parametrize("case", ALL_CASES, ids=sr.shape_id)
def test_jvp_against_float64(case):
    r = _reference(case)
    fused = r["fused"]
    worst = 0.0
    for M in sr.shape_rows(len(r["keys"]))[1:]:
        A, B = _jac(r, M)
        _, saved = fused.forward_saved(_kdev(r["keys"][:M]))
        k = M // 2
        v = _f32(np.random.RandomState(13).normal(size=A.shape[1])).astype(np.float64)
        ua, up = _jvp(fused, saved, v)
        ra, _ = _jvp(fused, saved, A[k])
        _, rp = _jvp(fused, saved, B[k])
        for u, J, vv in ((ua, A, v), (up, B, v), (ra, A, _f32(A[k]).astype(np.float64)), (rp, B, _f32(B[k]).astype(np.float64))):
            assert u.shape == (M,) and np.isfinite(u).all()
            err = spring.jvp_err(u, J, vv)
            worst = max(worst, err)
            assert err <= C_JVP_SHAPES, (case, M, err)
        assert ra[k] > 0 and rp[k] > 0
    cid = sr.shape_id(case)
    print(f"\n[sr shapes jvp] {cid}: worst |u - J64 v| / (|J64| |v|) {worst:.3e} (float32 CPU {JVP_F32[cid]:.3e}, bound {C_JVP_SHAPES:.2e})")


# ------------------------------------------------------------------------------------------------------ 3. map, tensor by tensor
@pytest.mark.parametrize("case", MAP_CASES, ids=sr.shape_id)
def test_every_parameter_tensor_meets_its_own_layer(case):
    r = _reference(case)
    M = 65
    A, B = _jac(r, M)
    _, saved = r["fused"].forward_saved(_kdev(r["keys"][:M]))
    v = _f32(np.random.RandomState(13).normal(size=A.shape[1])).astype(np.float64)
    names = [n for n, _ in r["w64"].model.named_parameters()]
    depth = len(case[3]) + 1
    assert sum(n.startswith("phase_layers.0.") for n in names) == 2 * depth, names
    off, worst = 0, 0.0
    for name, p in r["w64"].model.named_parameters():
        e = np.zeros_like(v)
        e[off:off + p.numel()] = v[off:off + p.numel()]
        off += p.numel()
        ua, up = _jvp(r["fused"], saved, e)
        for u, J in ((ua, A), (up, B)):
            err = spring.jvp_err(u, J, e)
            worst = max(worst, err)
            assert err <= C_JVP_SHAPES, (name, err)
        # a tensor that moves a block moves it here too, and no other (pair 0's first-layer weights meet the constant-zero input)
        assert (np.abs(ua).max() > 0) == (np.abs(A @ e).max() > 0) and (np.abs(up).max() > 0) == (np.abs(B @ e).max() > 0), name
    assert off == len(v)
    print(f"\n[sr shapes map] {sr.shape_id(case)}: {len(names)} tensors, worst {worst:.3e} (bound {C_JVP_SHAPES:.2e})")


# ------------------------------------------------------------------------------------------------------------- 4. direction
@pytest.mark.parametrize("case", DIRECTION_CASES, ids=sr.shape_id)
def test_direction_against_float64(case):
    r = _reference(case)
    M = len(r["keys"])
    kd, w, g = _leading(r, M)
    A, B = _jac(r, M)
    d, _ = tg._direction(r["fused"], kd, w, g)
    torch.cuda.synchronize()
    d = d.double().cpu().numpy()
    g64 = g.astype(np.float64)
    d64 = sr.direction(A, B, w, g64, SHIFT)
    grad64 = A.T @ g64[:, 0] + B.T @ g64[:, 1]
    err, who = sr.per_tensor_worst(r["w64"], d, d64)
    cid = sr.shape_id(case)
    c2 = 4 * DIRECTION_F32[cid]
    print(f"\n[sr shapes direction] {cid} M={M}: per-tensor error {err:.3e} at {who} (float32 CPU {DIRECTION_F32[cid]:.3e}, "
          f"bound {c2:.2e}), d.grad64 {d @ grad64:.3e}")
    assert np.isfinite(d).all() and err <= c2, (case, err, who)
    assert d @ grad64 > 0


# ------------------------------------------------------------------------------------------------- 5. orderings, bit for bit
def _ordered_pair(i, o):
    """CASES[i]'s handle at -1 with its table (test_sr_gpu._reference: held to float64 there), and a handle at ordering ``o`` with
    the same parameters and the keys that show it the same model-order bits."""
    case = sr.CASES[i]
    r = tg._reference(case)
    hil = r["hil"]
    O = sr.order_of(o, hil.N // 2)
    _, wfB = sr.make_net(case, device="cuda", qubit_ordering=O)
    wfB.model.load_state_dict(r["wf"].model.state_dict())
    qA, qB = gr.q2m_of(-1, hil.N), gr.q2m_of(O, hil.N)
    assert [int(q) for q in r["wf"].qubit2model_permutation] == qA and [int(q) for q in wfB.qubit2model_permutation] == qB and qA != qB
    keysB = gr.relabel_keys(r["keys"], qA, qB)
    assert not np.array_equal(keysB, r["keys"].astype(np.uint64)) and np.all(hil.is_physical(keysB))
    return r, _handle(wfB, (case, o)), keysB


def _everything(fused, keys, w, g, v):
    kd = _kdev(keys)
    _, saved = fused.forward_saved(kd)
    Ga, Gp = fused.sr_gram(saved, None, None, None, uncentred=True)
    wd = _dev(w)
    Ta, Tp, ya, yp = fused.sr_gram(saved, wd, _dev(g, torch.float32), SHIFT)
    ua, up = fused.sr_jvp(saved, v)
    d = fused.sr_direction(saved, wd, tg._solve(Ta, ya), tg._solve(Tp, yp))
    torch.cuda.synchronize()
    return dict(G_a=Ga, G_phi=Gp, T_a=Ta, T_phi=Tp, y_a=ya, y_phi=yp, u_a=ua, u_phi=up, d=d)


@pytest.mark.parametrize("i,o", sr.ORDER_CASES, ids=[f"{sr.case_id(sr.CASES[i])}-order_{o}" for i, o in sr.ORDER_CASES])
def test_orderings_give_the_bits_of_the_default_ordering(i, o):
    r, fB, keysB = _ordered_pair(i, o)
    M = len(r["keys"])
    _, w, g, _, _ = tg._leading(r, M)
    v = torch.as_tensor(_f32(np.random.RandomState(13).normal(size=r["A"].shape[1])), device="cuda")
    a = _everything(r["fused"], r["keys"], w, g, v)
    b = _everything(fB, keysB, w, g, v)
    for name in a:
        assert float(a[name].abs().max()) > 0 and torch.equal(a[name], b[name]), (i, o, name)


def test_spring_step_at_an_ordering_gives_the_bits_of_the_default_ordering():
    """One SPRING step through the optimiser's natural-gradient path (``_natural_gradient_update``), mu = 0.9, a fixed table and a
    fixed previous step: LiH single [64, 64] at the seeded pair permutation against the -1 handle."""
    from naqs_amd.optimizer import PartialSamplingOptimizer
    r, fB, keysB = _ordered_pair(5, "pi")
    M = len(r["keys"])
    _, w, g, _, _ = tg._leading(r, M)
    prev = _f32(1e-2 * np.random.RandomState(17).normal(size=r["A"].shape[1]))
    steps = []
    for fused, keys in ((r["fused"], r["keys"]), (fB, keysB)):
        class Wf:                                           # the step goes to a scratch vector, not to the shared network
            p = torch.zeros(fused.n_params, dtype=torch.float32, device="cuda")

            def flatten_parameters(self):
                return self.p

        opt = object.__new__(PartialSamplingOptimizer)
        opt.natural_gradient, opt.wavefunction = dict(diag_shift=SHIFT, lr=1.0, momentum=MU), Wf()
        opt._sr_phi_prev = torch.as_tensor(prev, device="cuda")
        _, saved = fused.forward_saved(_kdev(keys))
        opt._natural_gradient_update(fused, saved, _dev(w), _dev(g, torch.float32))
        torch.cuda.synchronize()
        assert opt.sr_last["momentum"] == MU and float(opt.sr_last["jvp_norm"]) > 0
        steps.append((opt._sr_phi_prev.clone(), Wf.p.clone()))
    assert not torch.equal(steps[0][0], torch.as_tensor(np.float32(MU) * prev, device="cuda"))
    assert torch.equal(steps[0][0], steps[1][0]) and torch.equal(steps[0][1], steps[1][1])


# ----------------------------------------------------------------------------------------------------- 6. the padding columns
def _gram_and_jvp(fused, keys, v):
    kd = _kdev(keys)
    _, saved = fused.forward_saved(kd)
    Ga, Gp = fused.sr_gram(saved, None, None, None, uncentred=True)
    ua, up = fused.sr_jvp(saved, v)
    torch.cuda.synchronize()
    return kd, saved, (Ga, Gp, ua, up)


def _destroy(wf):
    wf._fused.close()
    wf._fused = None


def test_padding_columns_are_zero_whatever_ran_before():
    """sr_gram_kernel and sr_jvp_kernel read 64 columns of [48]'s deltas and activations, 16 of them padding.  The same bits (a)
    after [512, 512] filled the device's memory with its own factors, (b) on a new handle once both are destroyed (what the
    allocator hands back is no longer fresh), (c) after a training backward with random seeds on the same handle and table."""
    big, small = _LIH[(512, 512)], _LIH[(48,)]
    rb, rs = _reference(big), _reference(small)
    keys = rs["keys"]
    M = len(keys)
    vb = torch.as_tensor(_f32(np.random.RandomState(13).normal(size=rb["J"].shape[1])), device="cuda")
    vs = torch.as_tensor(_f32(np.random.RandomState(13).normal(size=rs["J"].shape[1])), device="cuda")
    _, wf_big = sr.shape_net(big)
    _, wf_small = sr.shape_net(small)
    f_big, f_small = _handle(wf_big, big), _handle(wf_small, small)
    _, _, out_big = _gram_and_jvp(f_big, rb["keys"], vb)
    assert all(torch.isfinite(t).all() and float(t.abs().max()) > 0 for t in out_big)
    _, _, first = _gram_and_jvp(f_small, keys, vs)
    _destroy(wf_big)
    _destroy(wf_small)
    del f_big, f_small, wf_big, wf_small, out_big
    _, wf_new = sr.shape_net(small)
    f_new = _handle(wf_new, small)
    kd, saved, second = _gram_and_jvp(f_new, keys, vs)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    # the shared reference's handle, whatever ran on it before, agrees too
    _, _, shared = _gram_and_jvp(rs["fused"], keys, vs)
    assert all(torch.equal(a, b) for a, b in zip(first, shared))
    # a training step leaves nothing in the columns the Gram kernel reads
    seeds = torch.as_tensor(np.random.RandomState(19).normal(size=(M, 2)).astype(np.float32), device="cuda")
    grad = torch.empty(f_new.n_params, dtype=torch.float32, device="cuda")
    st = f_new._lib.naqs_net_train_backward(f_new._h, M, kd.data_ptr(), seeds.data_ptr(), grad.data_ptr(), _stream_ptr(f_new.device))
    assert st == 0
    Ga, Gp = f_new.sr_gram(saved, None, None, None, uncentred=True)
    ua, up = f_new.sr_jvp(saved, vs)
    torch.cuda.synchronize()
    assert float(grad.abs().max()) > 0 and all(torch.equal(a, b) for a, b in zip(second, (Ga, Gp, ua, up)))
    _destroy(wf_new)


# ----------------------------------------------------------------------------------------------------------- 7. determinism
@pytest.mark.parametrize("case", DETERMINISM_CASES, ids=sr.shape_id)
def test_same_bits_twice_and_at_any_table_that_holds_the_row(case):
    r = _reference(case)
    fused = r["fused"]
    M = len(r["keys"])
    kd, w, g = _leading(r, M)
    v = torch.as_tensor(_f32(np.random.RandomState(13).normal(size=r["J"].shape[1])), device="cuda")
    first, second = _everything(fused, r["keys"], w, g, v), _everything(fused, r["keys"], w, g, v)
    assert all(torch.equal(first[k], second[k]) for k in first)
    _, saved = fused.forward_saved(_kdev(r["keys"][:65]))
    part = fused.sr_jvp(saved, v)
    assert M > 65 and torch.equal(first["u_a"][:65], part[0]) and torch.equal(first["u_phi"][:65], part[1])
