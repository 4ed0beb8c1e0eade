"""The natural-gradient kernels at every phase shape the handle accepts, the part that needs no GPU: the yardsticks the bounds of
tests/test_sr_shapes_gpu.py come from, recomputed here and held against the figures recorded there.  Nothing is fixed in advance.

Per case of ``sr_reference.SHAPE_CASES`` and ``SYM_CASES`` (one network, one kink-free table of at most 130 rows, seeds recorded in
``sr_reference.SEEDS``), the float32 PyTorch network on the CPU against its float64 copy:

* ``GRAM_F32``       ``sr_reference.gram_err`` of J32 J32^T (float32 Jacobian rows, the products in float64) against J64 J64^T, the
                     worse of the two blocks on the whole table — exactly as test_sr_gpu.py defines its own figure;
* ``JVP_F32``        ``spring_reference.jvp_err`` of J32 v (product in float64) over both blocks, M = 65 and 130 leading rows and the
                     two operands of test_sr_momentum_gpu._jvp_case: a seeded normal v and the float32-rounded row M // 2 of J64;
* ``DIRECTION_F32``  ``sr_reference.direction_f32``'s per-tensor error at the whole table, for the cases the direction test runs.

C_SHAPES = max(test_sr_gpu.C, 4 x the worst GRAM_F32) and C_JVP_SHAPES = max(test_sr_momentum_gpu.C_JVP, 4 x the worst JVP_F32);
4 x is the margin the existing natural-gradient bounds sit at over their CPU figures, and the kernels' MFMA sums are float64, so
they should land on the float32 network's error and not above it.  The float32 network is the only yardstick: were a deep shape's
figure much larger than the existing yardstick, 4 x that figure would be that shape's bound and no other's.  None is: the worst
Gram figure over the new cases is 1.26e-7 (LiH [512] * 3; [16] * 8 and [64] * 8: 8.0e-8 and 6.5e-8, the amplitude block's) against
the 1.70e-7 of the existing cases, so C_SHAPES is test_sr_gpu.C, 6.8e-7, unchanged; the worst JVP figure is 8.63e-8 (LiH
[160, 32], the seeded normal v on the phase block) against 5.84e-8, so C_JVP_SHAPES = 3.45e-7 for every shape.  The direction's
figures run from 2.6e-5 ([48]) to 6.1e-4 ([16] * 8) and are per case, as in test_sr_gpu.py.

Each test recomputes its case's figures and asserts that the recorded ones are within 10 % of them and that the table holds
``sr_reference.rows_wanted`` kink-free rows: a stale constant fails here, without a GPU.
"""
import numpy as np
import pytest

import grad_reference as gr
import spring_reference as spring
import sr_reference as sr

torch = pytest.importorskip("torch")

SHIFT = 1e-2                      # test_sr_gpu.SHIFT
ALL_CASES = sr.SHAPE_CASES + sr.SYM_CASES


def direction_cases():
    """(48,), (100, 200), (512, 512) at both amplitude widths and (16,) * 8 on LiH, and every symmetric case."""
    shapes = {(48,), (100, 200), (512, 512), (16,) * 8}
    return [c for c in sr.SHAPE_CASES if c[0] == "LiH" and c[3] in shapes] + sr.SYM_CASES


def jvp_operands(A, B, M):
    """test_sr_momentum_gpu._jvp_case's operands for the leading M rows -> [(block J, v float64 holding float32 values)]."""
    k = M // 2
    v = np.random.RandomState(13).normal(size=A.shape[1]).astype(np.float32).astype(np.float64)
    return [(0, v), (1, v), (0, A[k].astype(np.float32).astype(np.float64)), (1, B[k].astype(np.float32).astype(np.float64))]


def seeds_e(n):
    rs = np.random.RandomState(7)          # test_sr_gpu._reference's local energies
    return rs.normal(-7.0, 1.0, n) + 1j * rs.normal(0.0, 0.3, n)


def measure(case, with_direction):
    hil, wf = sr.shape_net(case, device="cpu")
    _, w64 = gr.f64_copy(wf)
    _, w32 = gr.f64_copy(wf, torch.float32)
    keys, w = sr.table(hil, w64, rows=sr.SHAPE_TABLE)
    st = sr.states_of(hil, keys)
    A, B = sr.jacobians(w64, st)
    A32, B32 = sr.jacobians(w32, st)
    out = dict(rows=len(keys), wanted=sr.rows_wanted(hil), size=hil.size, n_params=A.shape[1])
    out["gram"] = max(sr.gram_err(J32 @ J32.T, J @ J.T) for J32, J in ((A32, A), (B32, B)))
    out["jvp"] = 0.0
    for M in sr.shape_rows(len(keys))[1:]:
        for blk, v in jvp_operands(A, B, M):
            J32, J = ((A32, A), (B32, B))[blk]
            out["jvp"] = max(out["jvp"], spring.jvp_err(J32[:M] @ v, J[:M], v))
    if with_direction:
        g = gr.loss_grad_f64(seeds_e(len(keys)), w).astype(np.float32)
        d64 = sr.direction(A, B, w, g.astype(np.float64), SHIFT)
        out["direction"] = sr.per_tensor_err(w64, sr.direction_f32(w32, st, A32, B32, w, g, SHIFT), d64)
    return out


def test_case_tables_are_what_the_issue_lists():
    ids = [sr.shape_id(c) for c in ALL_CASES]
    assert len(set(ids)) == len(ids) == 27
    assert {c[3] for c in sr.SHAPE_CASES if c[0] == "LiH" and c[2] == 16} == {ph for ph, _ in sr._SHAPES} and len(sr._SHAPES) == 13
    assert all(c[4] and gr.sector(c[0]) for c in sr.SYM_CASES) and not any(c[4] for c in sr.SHAPE_CASES)
    assert sorted(c[5] for c in sr.SYM_CASES if c[1]) == ["FULL", "FULL", "PARTIAL", "PARTIAL"]
    assert all(c in ALL_CASES for c in direction_cases()) and len(direction_cases()) == 5 + len(sr.SYM_CASES)
    assert [sr.CASES[i][:2] for i, _ in sr.ORDER_CASES[::2]] == [("LiH", False), ("LiH", True), ("syn32_8_8", False)]
    for i, o in sr.ORDER_CASES:
        N = gr.sector(sr.CASES[i][0])[1]
        q = gr.q2m_of(sr.order_of(o, N // 2), N)
        assert sorted(q) == list(range(N)) and q != gr.q2m_of(-1, N) and (o == 1) == (q == gr.q2m_of(1, N))


def test_bounds_are_four_times_the_worst_recorded_figure():
    import test_sr_gpu as tg
    import test_sr_momentum_gpu as tm
    import test_sr_shapes_gpu as ts
    ids = {sr.shape_id(c) for c in ALL_CASES}
    assert set(ts.GRAM_F32) == set(ts.JVP_F32) == ids and set(ts.DIRECTION_F32) == {sr.shape_id(c) for c in direction_cases()}
    assert ts.C_SHAPES == max(tg.C, 4 * max(ts.GRAM_F32.values())) and ts.C_JVP_SHAPES == max(tm.C_JVP, 4 * max(ts.JVP_F32.values()))
    assert ts.SHIFT == tg.SHIFT == SHIFT
    # no shape's float32 figure is "much larger" than the existing yardstick: one constant for all (the module docstring)
    assert max(ts.GRAM_F32.values()) < 2 * tg.C / 4 and max(ts.JVP_F32.values()) < 2 * tm.C_JVP / 4


@pytest.mark.parametrize("case", ALL_CASES, ids=sr.shape_id)
def test_recorded_yardsticks_are_what_the_float32_network_gives(case):
    import test_sr_shapes_gpu as ts
    cid = sr.shape_id(case)
    m = measure(case, case in direction_cases())
    print(f"\n[sr shapes yardstick] {cid}: rows {m['rows']} (wanted {m['wanted']} of {m['size']}), N_p {m['n_params']}, "
          f"gram {m['gram']:.3e}, jvp {m['jvp']:.3e}, direction {m.get('direction', float('nan')):.3e}")
    assert m["wanted"] <= m["rows"] <= sr.SHAPE_TABLE, (cid, m)
    assert m["gram"] > 0 and abs(ts.GRAM_F32[cid] - m["gram"]) <= 0.1 * m["gram"], (cid, ts.GRAM_F32[cid], m["gram"])
    assert m["jvp"] > 0 and abs(ts.JVP_F32[cid] - m["jvp"]) <= 0.1 * m["jvp"], (cid, ts.JVP_F32[cid], m["jvp"])
    if "direction" in m:
        assert abs(ts.DIRECTION_F32[cid] - m["direction"]) <= 0.1 * m["direction"], (cid, ts.DIRECTION_F32[cid], m["direction"])
