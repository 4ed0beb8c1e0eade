"""The natural-gradient step at the table sizes of a run on N2 (1 000 to 4 300 rows), the parts that need no GPU: the yardsticks
the bounds of tests/test_sr_scale_gpu.py come from, recomputed, and its measures rehearsed on code known to be right.

1. The float32 CPU network's Gram error on the sampled rows of ``sr_reference.LARGE_CASES`` (float32 Jacobian rows, products in
   float64, against float64 rows): 7.1e-8 / 8.3e-8, 5.8e-8 / 2.5e-8 and 6.2e-8 / 1.08e-7 (amplitude / phase) — inside the 1.70e-7
   that test_sr_gpu.C is four times of, so C holds for the new cases as it stands.  The same for ``WIDTH_CASES``' full tables.
2. The direction's yardstick per width case (sr_reference.direction_f32 against the float64 direction), held against the
   table ``DIRECTION_YARDSTICK`` that test_sr_scale_gpu.py takes its bounds from.
3. X^T x is the backward pass with the seeds of ``sr_reference.seeds_f64``: the reference of the GPU module's direction test.
4. ``sr_solve_reference.rho_rows``, ``eta`` and ``fwd`` at M = 1 025 on LAPACK and on the float64 blocked model of the kernels:
   inside the bounds the GPU module applies; with one float32 rounding, outside.
"""
import numpy as np
import pytest

import grad_reference as gr
import sr_reference as sr
import sr_solve_reference as ss

torch = pytest.importorskip("torch")

GRAM_YARDSTICK = 1.70e-7          # test_sr_gpu.C = 4 x this (the float32 CPU network's worst case over sr_reference.CASES)
SHIFT = 1e-2                      # test_sr_gpu.SHIFT

# The float32-CPU pipeline's per-tensor direction error (sr_reference.direction_f32) per width case on the whole table of 200 rows,
# as this module computes it (test 2); tests/test_sr_scale_gpu.py bounds the kernels' direction by 4 x these.  Not at the 65
# leading rows: the keys ascend, the leading rows share the first model pair's occupation, the centring takes that block's direction
# to zero, and a per-tensor relative error of a tensor that is zero but for rounding says nothing (test_sr_gpu.py measures the
# direction on whole tables for the same reason).
DIRECTION_YARDSTICK = {
    "LiH-single-a32-p32-sym-PARTIAL": 1.509e-04,
    "LiH-single-a48-p32-sym-PARTIAL": 1.613e-04,
    "LiH-single-a96-p32-sym-PARTIAL": 2.232e-04,
    "LiH-single-a128-p32-sym-PARTIAL": 1.993e-04,
    "LiH-agg-a32-p32-sym-PARTIAL": 1.136e-04,
    "LiH-agg-a48-p32-sym-PARTIAL": 1.344e-04,
    "LiH-agg-a96-p32-sym-PARTIAL": 9.293e-05,
    "LiH-agg-a128-p32-sym-PARTIAL": 2.447e-04,
}


def _nets(case):
    hil, wf = sr.make_net(case, device="cpu")
    _, w64 = gr.f64_copy(wf)
    _, w32 = gr.f64_copy(wf, torch.float32)
    return hil, w64, w32


def _gram_f32_err(J32, J64):
    return sr.gram_err(J32 @ J32.T, J64 @ J64.T)


# ------------------------------------------------------------------------------------------------ 1. the Gram yardstick
def test_the_gram_bound_is_four_times_the_yardstick():
    import test_sr_gpu as tg
    assert tg.C == 4 * GRAM_YARDSTICK and tg.SHIFT == SHIFT


@pytest.mark.parametrize("case", sr.LARGE_CASES, ids=sr.case_id)
def test_float32_cpu_gram_on_the_sampled_rows(case):
    hil, w64, w32 = _nets(case)
    keys, w = sr.table(hil, w64, rows=sr.LARGE_ROWS)
    assert len(keys) == sr.LARGE_ROWS and np.all(np.diff(keys.astype(np.uint64)) > 0) and abs(w.sum() - 1) < 1e-12
    if case[0] == "syn32_8_8":
        assert (keys.astype(np.uint64) >> np.uint64(31)).max() == 1          # bit 31 of the keys is in use
    R = sr.sampled_rows()
    assert set(sr.FIXED_ROWS) <= set(R.tolist()) and len(R) >= 64 and R.max() == sr.LARGE_ROWS - 1
    for M in sr.LARGE_SIZES:
        rows, pos = sr.rows_below(R, M)
        assert rows[-1] == M - 1 and np.array_equal(R[pos], rows)
    st = sr.states_of(hil, keys[R])
    A, B = sr.jacobians(w64, st)
    A32, B32 = sr.jacobians(w32, st)
    ea, ep = _gram_f32_err(A32, A), _gram_f32_err(B32, B)
    print(f"\n[sr scale yardstick] {sr.case_id(case)}: float32 CPU |G32 - G64| on {len(R)} sampled rows: amplitude {ea:.3e}, "
          f"phase {ep:.3e} (yardstick {GRAM_YARDSTICK:.2e})")
    assert 0 < ea <= GRAM_YARDSTICK and 0 < ep <= GRAM_YARDSTICK, (case, ea, ep)


# ----------------------------------------------------------------------------------------- 2. the direction's yardstick
@pytest.mark.parametrize("case", sr.WIDTH_CASES, ids=sr.case_id)
def test_width_cases_yardsticks(case):
    """Per width case: the float32 CPU network's Gram error on the full table is inside the yardstick C comes from, and its
    direction error is the one committed in DIRECTION_YARDSTICK.  The latter is set by cancellation in a float32 backward,
    whose summation order belongs to the BLAS underneath: within a factor of two either way counts as the same figure."""
    hil, w64, w32 = _nets(case)
    keys, w_all = sr.table(hil, w64)
    assert len(keys) == max(sr.WIDTH_ROWS)
    st = sr.states_of(hil, keys)
    A, B = sr.jacobians(w64, st)
    A32, B32 = sr.jacobians(w32, st)
    ea, ep = _gram_f32_err(A32, A), _gram_f32_err(B32, B)
    assert 0 < ea <= GRAM_YARDSTICK and 0 < ep <= GRAM_YARDSTICK, (case, ea, ep)
    rs = np.random.RandomState(7)
    e = rs.normal(-7.0, 1.0, len(keys)) + 1j * rs.normal(0.0, 0.3, len(keys))
    g = gr.loss_grad_f64(e, w_all).astype(np.float32)
    d64 = sr.direction(A, B, w_all, g.astype(np.float64), SHIFT)
    got = sr.per_tensor_err(w64, sr.direction_f32(w32, st, A32, B32, w_all, g, SHIFT), d64)
    print(f"\n[sr scale yardstick] {sr.case_id(case)}: float32 CPU |G32 - G64| amplitude {ea:.3e}, phase {ep:.3e}; direction_f32 "
          f"at M = {len(keys)}: {got:.3e}")
    want = DIRECTION_YARDSTICK[sr.case_id(case)]
    assert 0.5 * want <= got <= 2 * want, (case, got, want)


# --------------------------------------------------------------------------------- 3. the direction as a backward pass
@pytest.mark.parametrize("case", [sr.CASES[4], sr.CASES[6]], ids=sr.case_id)
def test_direction_is_the_backward_pass_of_the_seeds(case):
    """X^T x = sum_i s_i d log psi_i / d theta with s = seeds_f64(w, x), per block, in float64."""
    hil, w64, _ = _nets(case)
    keys, w = sr.table(hil, w64, rows=40)
    st = sr.states_of(hil, keys)
    A, B = sr.jacobians(w64, st)
    rs = np.random.RandomState(2)
    xa, xp = rs.normal(size=len(keys)), rs.normal(size=len(keys))
    want = sr.system(A, w, w, SHIFT)[2].T @ xa + sr.system(B, w, w, SHIFT)[2].T @ xp
    seeds = np.stack([sr.seeds_f64(w, xa), sr.seeds_f64(w, xp)], -1)
    got = sr.flat(w64, gr.grad_f64(w64, st, seeds))
    assert np.abs(want).max() > 0 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ------------------------------------------------------------------------------------ 4. the solve's measures at 1 025
def test_rho_rows_is_rho_on_the_rows_it_is_given():
    (T, y), _ = ss.pair(200, 1e-3)
    _, L, info = ss.blocked_model(T, y)
    assert info == 0
    full = ss.rho(T, L)
    assert ss.rho_rows(T, L, np.arange(200)) == pytest.approx(full, rel=1e-12)
    assert 0 < ss.rho_rows(T, L, [0, 63, 64, 199]) <= full
    # the strict upper triangle is ignored
    assert ss.rho_rows(T, L + np.triu(np.ones_like(L), 1), [0, 63, 64, 199]) == ss.rho_rows(T, L, [0, 63, 64, 199])


def test_measures_at_1025_rows_pass_for_lapack_and_the_blocked_model():
    from scipy.linalg import lapack
    M = 1025
    rows = [0, 63, 64, 511, 512, 960, 1023, 1024]
    for T, y in ss.pair(M, 1e-3):
        x_ref, info_ref = ss.lapack_solve(T, y)
        x, L, info = ss.blocked_model(T, y)
        assert info == info_ref == 0
        ev = np.linalg.eigvalsh(T)
        cond = ev[-1] / ev[0]
        assert ev[0] > 0
        L_ref = np.tril(lapack.dpotrf(T, lower=1)[0])
        for xs, Ls in ((x, L), (x_ref, L_ref)):
            e, r = ss.eta(T, xs, y), ss.rho_rows(T, Ls, rows)
            assert e <= ss.bound(M) and r <= ss.bound(M), (e, r)
        f = ss.fwd(x, x_ref)
        print(f"\n[sr scale rehearsal] M={M}: blocked model eta {ss.eta(T, x, y):.3e}, rho_rows {ss.rho_rows(T, L, rows):.3e} (bound "
              f"{ss.bound(M):.2e}), fwd {f:.3e} (bound {cond * ss.bound(M):.2e}, cond_2 {cond:.2e})")
        assert f <= cond * ss.bound(M)
        # one float32 rounding is outside
        assert ss.eta(T, x.astype(np.float32), y) > ss.bound(M)
        assert ss.rho_rows(T, L.astype(np.float32), rows) > ss.bound(M)
