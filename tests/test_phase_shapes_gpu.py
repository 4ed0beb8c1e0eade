"""The single phase MLP against float64 at every width and depth class the library accepts (1..8 hidden layers of 1..512 units).

The other float64 suites run the MLP at [512, 512] (and [64, 64] in one backward case).  phase_kernel_h / phase_kernel
(naqs_logpsi.hip) branch on the padded widths of every layer: N_pad = pad16(N) selects the K-split arm of mlp_layer_h
(N_pad == 16), the interleaved write-back (N_pad % 64 == 0) or the plain one with a ragged last wave; Kh_pad = pad32(K) of the
NEXT layer decides whether 16 columns of the activation tile lie between what one layer writes and the next one reads (N_pad an
odd multiple of 16); pack_phase_* zero-pad weights and bias of widths that are no multiple of 16; layer 0 takes the pre-fetched
form when it is 512 wide with a next layer.  SHAPES names the branch each shape is here for.

Per (shape, sector) the forward runs at 1, 15, 16, 17 rows and the whole key set (whole sector, or 2 000 random keys, plus a
quarter as many unphysical keys under PARTIAL masking), with NAQS_PHASE_RB = 1..4 (the tile height, which otherwise needs over
4 096 rows to leave 1) in NAQS_PHASE_MODE = 2, 1, 0: no NaN, log|psi| and phase within test_forward_f64_gpu.py's bounds of the
float64 copy (phase scale: the whole key set's, as test_pairs_gpu._compare), forward_saved the same bits (modes 2, 1), the kernel
name select_form's rules give (never phase_kernel_ws).  test_forward_after_a_wider_network re-packs a narrow network after a
[512, 512] one ran on the device (what the LDS held before must not matter).  The backward: test_pairs_gpu._check_backward (both
call forms bit for bit, each tensor within BOUND of its scale of the float64 gradient), kink rows counted on the CPU first
(<= 10 % of every row count).  One training case: 50 library steps at [16, 16] on LiH, then the whole space against the float64
copy of the trained parameters.

Bounds.  Depth <= 2: LOG_PAIR, LOG_REL, PHASE_REL, PHASE_FLOOR of test_forward_f64_gpu.py and BOUND, TAU of test_backward_gpu.py,
unchanged.  Depth 3..8 had no phase bound: PHASE_REL_DEEP[depth] = max(PHASE_REL, 4 x the worst |float32 CPU copy - float64|
phase error at that depth over this module's (shape, sector) cases, in units of max(PHASE_FLOOR, largest |phase|)) — 4 x because
the split formats carry a few more roundings per product than plain float32, the ratio at which the existing bounds sit over
the CPU figures the suite prints.  Measured on the CPU (float32 copy, networks of the seeds below):
    depth 3: [32, 32, 32] 2.6e-8 (H2) 1.09e-7 (LiH) 1.43e-7 (LiF), [512, 512, 512] 1.23e-7 (H2) 3.12e-7 (LiH) 4.40e-7 (LiF)
             -> 4 x 4.40e-7 = 1.76e-6 < PHASE_REL: the floor, 5e-6, is the bound
    depth 8: [64] * 8 4.7e-8 (H2) 1.14e-7 (LiH) 1.18e-7 (LiF), [16] * 8 6.1e-8 (H2) 6.5e-8 (LiH) 9.0e-8 (LiF)
             -> 4 x 1.18e-7 = 4.7e-7 < PHASE_REL: the floor, 5e-6, is the bound
(depth 1 and 2, for comparison: worst 3.9e-7 and 5.2e-7).  A default-initialised deep MLP's phases err no more than a shallow
one's: every depth keeps 5e-6.  profiles/phase_shapes.txt has every case's figures, CPU and MI355X.  No accepted shape is
refused by the backward: its only NAQS_ERR_UNSUPPORTED exit (the LDS of backward_mega_kernel) depends on the amplitude width
alone, and test_backward_against_float64 asserts the handle trains on the HIP path for each of its shapes.

Measured on an MI355X (the whole module: 9 s): worst HIP error 0.30 of the bound in the forward (log|psi| at LiF; the phase at most
0.29 of its bound, [64] * 8 on LiH in the f16x2 format: 2.05e-7), 0.10 in the backward ([16] * 8; 0.03 elsewhere), kink rows at
most 2.3 % of a row count.  Without mlp_zero_gap_h (naqs_logpsi.hip) 37 forward cases of the shapes whose N_pad is an odd
multiple of 16 return NaN phases, and seven backward cases and the training case fail (profiles/phase_shapes.txt).
"""
import math

import numpy as np
import pytest

import grad_reference as gr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# label -> (phase_hidden, phase_sym, sectors, the branch it is here for)
_A = "<= 16 outputs in a hidden layer: mlp_layer_h's ncb == 1 arm (waves split K), not last"
_B = "N_pad an odd multiple of 16: 16 unwritten columns before the next layer's Kh_pad"
_C = "width no multiple of 16: zero-padded weights and bias (pack_phase_f32 / _f16 / _bf16)"
_D = "N_pad no multiple of 64: plain write-back (inter false), ragged last wave (my_cb = 1, 2, 3)"
_E = "multiples of 64 other than 512: interleaved column map (tile_col), inter write-back"
_F = "512 first with a next layer: mlp_layer0_pre (pre0); [512] alone has n_lin == 2; 512 not first: pre0 false"
_G = "depth 3..8"
SHAPES = {
    "16": ((16,), False, ("H2", "LiH", "LiF"), _A),
    "16x2": ((16, 16), False, ("H2", "syn6_2_1", "LiH", "LiF"), _A),
    "1": ((1,), False, ("H2", "LiH", "LiF"), _A),
    "8x2": ((8, 8), False, ("H2", "LiH", "LiF"), _A),
    "512_16": ((512, 16), False, ("H2", "LiH", "LiF"), _A + "; K = 512 split over all 8 waves"),
    "16_512": ((16, 512), False, ("H2", "LiH", "LiF"), _A + ", then 512 columns read the 32-column tile"),
    "48": ((48,), False, ("H2", "syn6_2_1", "LiH", "LiF"), _B + " (my_cb = 3)"),
    "48_80": ((48, 80), False, ("H2", "LiH", "LiF"), _B + " (both layers)"),
    "496x2": ((496, 496), False, ("H2", "syn6_2_1", "LiH", "LiF"), _B + " (last wave my_cb = 3)"),
    "33": ((33,), False, ("H2", "LiH", "LiF"), _B + ", and " + _C),
    "5": ((5,), False, ("H2", "LiH", "LiF"), _C),
    "17x2": ((17, 17), False, ("H2", "LiH", "LiF"), _C + " (N_pad = 32: my_cb = 2)"),
    "100_200": ((100, 200), False, ("H2", "LiH", "LiF"), _C + " (N_pad 112, 208)"),
    "500": ((500,), False, ("H2", "LiH", "LiF"), _C + " (N_pad 512: inter)"),
    "80": ((80,), False, ("H2", "LiH", "LiF"), _D + ": wave 1 my_cb = 1"),
    "96x2": ((96, 96), False, ("H2", "LiH", "LiF"), _D + ": wave 1 my_cb = 2"),
    "112": ((112,), False, ("H2", "LiH", "LiF"), _D + ": wave 1 my_cb = 3"),
    "160_32": ((160, 32), False, ("H2", "LiH", "LiF"), _D + ": wave 2 my_cb = 2; wave 0 alone my_cb = 2"),
    "64x2": ((64, 64), False, ("H2", "LiH", "LiF"), _E),
    "128_256": ((128, 256), False, ("H2", "LiH", "LiF"), _E),
    "512": ((512,), False, ("H2", "LiH", "LiF"), _F),
    "64_512": ((64, 512), False, ("H2", "LiH", "LiF"), _F),
    "32x3": ((32,) * 3, False, ("H2", "LiH", "LiF"), _G),
    "64x8": ((64,) * 8, False, ("H2", "LiH", "LiF"), _G),
    "512x3": ((512,) * 3, False, ("H2", "LiH", "LiF"), _G + " (pre0, n_lin == 4: not phase_kernel_ws's shape)"),
    "16x8": ((16,) * 8, False, ("H2", "LiH", "LiF"), _G + ", every hidden layer through the ncb == 1 arm"),
    # -phase_sym (3 outputs, spin-ordered inputs, the sign shift): one of <= 16, one with the gap, one ragged
    "16x2_sym": ((16, 16), True, ("H2", "LiH", "LiF"), _A + ", -phase_sym"),
    "48_sym": ((48,), True, ("H2", "LiH", "LiF"), _B + ", -phase_sym"),
    "112_sym": ((112,), True, ("H2", "syn6_2_1", "LiH", "LiF"), _D + ", -phase_sym"),
}
FORWARD = [(s, n) for s, v in SHAPES.items() for n in v[2]]
# one shape per branch on LiH and LiF; the deepest and the narrowest on H2
BACKWARD = [(s, n) for s in ("16x2", "48_80", "100_200", "96x2", "128_256", "64_512", "32x3") for n in ("LiH", "LiF")] + \
           [("64x8", "H2"), ("16x2", "H2"), ("16x8", "LiH")]
SEEDS = {}                       # (shape, sector) -> seed where the default (the sector's P) puts too many rows on a kink
LIF_KEYS = 2000
ROWS = (1, 15, 16, 17)
MODES = ("2", "1", "0")
RBS = ("1", "2", "3", "4")
KINK_CAP = 0.1                   # test_backward_gpu.py's cap on rows within TAU of a ReLU kink

# phase bound per depth, in units of max(PHASE_FLOOR, largest |phase| of the key set): see the module docstring
PHASE_REL_DEEP = {3: 5e-6, 8: 5e-6}


def _phase_rel(depth):
    import test_forward_f64_gpu as tf
    return tf.PHASE_REL if depth <= 2 else PHASE_REL_DEEP[depth]


def _case_net(shape, name, device="cuda"):
    hidden, sym = SHAPES[shape][:2]
    P = gr.sector(name)[1] // 2
    return gr.sector_net(name, device=device, seed=SEEDS.get((shape, name), P), phase_sym=sym, phase_hidden=hidden)


def _case_keys(hil):
    """The whole sector (2 000 random keys of LiF's 44 100) plus a quarter as many unphysical keys, shuffled."""
    import test_pairs_gpu as tp
    phys = tp._whole(hil) if hil.size <= LIF_KEYS else gr.random_keys(hil, LIF_KEYS, 5)
    return np.random.RandomState(6).permutation(np.concatenate([phys, tp._unphysical(hil, max(1, len(phys) // 4), 7)]))


def _pad(x, m):
    return (x + m - 1) // m * m


def _expect(P, hidden, sym, M, save, mode, rb_env, cu):
    """naqs_net_last_kernel's string for M rows: layout_phase_mlp's ldh, phase_rb_max, select_form (naqs_logpsi.hip)."""
    import test_forward_f64_gpu as tf
    auto = max(1, math.ceil(M / (tf.TILE * cu)))
    if mode == 0:
        rb = rb_env if 1 <= rb_env <= tf.F32_RB_CAP else min(tf.F32_RB_CAP, auto)
        return f"phase_kernel<RB={rb}> (f32 MFMA) + amp_mfma_kernel<4>"
    K, widest = max(1, 2 * (P - 1)), 0
    for N in list(hidden) + [3 if sym else 4]:
        widest = max(widest, _pad(K, 32), _pad(N, 16))
        K = N
    slab = (2 if mode == 2 else 3) * tf.TILE * (widest + 8) * 2
    rb_max = min(tf.H_RB_CAP[mode], 155 * 1024 // slab)
    rb = rb_env if 1 <= rb_env <= rb_max else min(rb_max, auto)
    return f"phase_kernel_h<RB={rb}, SAVE={save}, FMT={mode} ({'f16x2' if mode == 2 else 'bf16x3'})> incl. amplitude prologue"


def _compare(got, want, P, scale, depth):
    """test_pairs_gpu._compare with the phase bound of ``depth`` -> (problems, |d| log, |d| phase, worst ratio to the bound)."""
    import test_forward_f64_gpu as tf
    import test_pairs_gpu as tp
    bad, e0, e1, _ = tp._compare(got, want, P, scale)
    r1 = e1 / (_phase_rel(depth) * max(tf.PHASE_FLOOR, scale))
    bad = [b for b in bad if not b.startswith("phase")] + ([f"phase {e1:.2e} ({r1:.2f} x bound)"] if not r1 <= 1 else [])
    g = np.asarray(got, np.float64)
    fin = np.isfinite(want[:, 0]) & np.isfinite(g[:, 0])
    r0 = (np.abs(g[fin, 0] - want[fin, 0]) / tf._bound_log(want[fin, 0], P)).max(initial=0.0)
    return bad, e0, e1, max(r0, r1)


def _references(hil, wf, keys):
    import test_pairs_gpu as tp
    _, wf64 = gr.f64_copy(wf)
    _, wf32 = gr.f64_copy(wf, dtype=torch.float32)
    st = tp._states(hil, keys)
    return gr.log_psi_f64(wf64, st), gr.log_psi_f64(wf32, st)


def _set_format(monkeypatch, fused, mode=None, rb=None):
    for k, v in (("NAQS_PHASE_MODE", mode), ("NAQS_PHASE_RB", rb)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    fused.refresh()                                      # (the number format is chosen when the weights are packed)


@pytest.mark.parametrize("shape,name", FORWARD)
def test_forward_against_float64(shape, name, monkeypatch):
    import test_forward_f64_gpu as tf
    import test_pairs_gpu as tp
    tp._threads()
    cu = tf._cus()
    hidden, sym = SHAPES[shape][:2]
    hil, wf = _case_net(shape, name)
    fused = wf.fused()
    assert fused is not None
    P, depth = hil.N // 2, len(hidden)
    keys = _case_keys(hil)
    ref64, ref32 = _references(hil, wf, keys)
    assert not np.isnan(ref64).any()
    scale = np.abs(ref64[:, 1]).max()
    _, c0, c1, rc = _compare(ref32, ref64, P, scale, depth)
    fails, worst = [], 0.0
    try:
        for mode in MODES:
            for rb in RBS:
                _set_format(monkeypatch, fused, mode, rb)
                w0 = w1 = wr = 0.0
                for m in sorted({r for r in ROWS if r <= len(keys)} | {len(keys)}):
                    ks, want = gr.sorted_rows(keys, m, ref64)
                    k_d = tp._kdev(ks)
                    lp = fused.log_psi(k_d).clone()
                    ran = fused.last_kernel()
                    bad, e0, e1, r = _compare(lp.cpu().numpy(), want, P, scale, depth)
                    w0, w1, wr = max(w0, e0), max(w1, e1), max(wr, r)
                    exp = _expect(P, hidden, sym, m, 0, int(mode), int(rb), cu)
                    if ran != exp or "phase_kernel_ws" in ran:
                        bad.append(f"ran {ran!r}, expected {exp!r}")
                    if mode != "0":                      # (the f32 kernel saves no activations: no training forward)
                        lpt, _ = fused.forward_saved(k_d)
                        if not torch.equal(lpt, lp):
                            bad.append("forward_saved differs from naqs_net_logpsi")
                        exp = _expect(P, hidden, sym, m, 1, int(mode), int(rb), cu)
                        if fused.last_kernel() != exp:
                            bad.append(f"training forward ran {fused.last_kernel()!r}, expected {exp!r}")
                    fails += [(mode, rb, m, b) for b in bad]
                worst = max(worst, wr)
                print(f"[phase shape {list(hidden)}{' sym' if sym else ''} {name} P={P}] MODE={mode} RB={rb} {ran}  |HIP - f64| log "
                      f"{w0:.2e} phase {w1:.2e} ({wr:.2f} x bound)")
    finally:
        _set_format(monkeypatch, fused)
    print(f"[phase shape {list(hidden)}{' sym' if sym else ''} {name} P={P}] M={len(keys)} max |phase| {scale:.2e}  worst HIP error "
          f"{worst:.2f} x bound  |torch f32 CPU - f64| log {c0:.2e} phase {c1:.2e} ({rc:.2f} x bound; phase / scale "
          f"{c1 / max(tf.PHASE_FLOOR, scale):.2e})")
    assert not fails, fails[:12]


@pytest.mark.parametrize("shape", ["16x2", "48", "17x2", "16x8"])
def test_forward_after_a_wider_network(shape, monkeypatch):
    """The activation tile of a narrow network lies in LDS that other kernels filled before: the same keys before and after a
    [512, 512] network of the sector ran on the device and the narrow one was packed again — the same bits, within the bounds."""
    import test_pairs_gpu as tp
    tp._threads()
    hidden, sym = SHAPES[shape][:2]
    hil, wf = _case_net(shape, "LiH")
    _, wide = gr.sector_net("LiH", seed=3)
    fused, fwide = wf.fused(), wide.fused()
    keys = np.sort(_case_keys(hil))
    ref64, _ = _references(hil, wf, keys)
    scale = np.abs(ref64[:, 1]).max()
    k_d = tp._kdev(keys)
    fails = []
    try:
        for mode in ("2", "1"):
            _set_format(monkeypatch, fused, mode, "1")
            _set_format(monkeypatch, fwide, mode, "1")
            first = fused.log_psi(k_d).clone()
            for _ in range(3):
                lw = fwide.log_psi(k_d)
                lw2, _ = fwide.forward_saved(k_d)
            assert torch.isfinite(lw[:, 1]).all() and torch.equal(lw, lw2)
            fused.refresh()
            second = fused.log_psi(k_d).clone()
            third, _ = fused.forward_saved(k_d)
            bad, e0, e1, r = _compare(second.cpu().numpy(), ref64, hil.N // 2, scale, len(hidden))
            print(f"[after a wider network {list(hidden)} LiH] MODE={mode} {fused.last_kernel()}  |HIP - f64| log {e0:.2e} phase {e1:.2e} "
                  f"({r:.2f} x bound)  same bits as before: {torch.equal(first, second)}")
            if not (torch.equal(first, second) and torch.equal(second, third)):
                bad.append("the bits depend on what ran before")
            fails += [(mode, b) for b in bad]
    finally:
        _set_format(monkeypatch, fused)
        _set_format(monkeypatch, fwide)
    assert not fails, fails


def _kink_rows(shape, name):
    """Rows within TAU of a ReLU kink at each row count _check_backward runs (the float64 copy, on the CPU)."""
    import test_pairs_gpu as tp
    from test_backward_gpu import TAU, W0_FUSE
    hil, wf = _case_net(shape, name, device="cpu")
    sizes = sorted({1, min(hil.size, 17), min(hil.size, 3000)} | ({W0_FUSE + 1} if hil.size > W0_FUSE else set()))
    keys = tp._keyset(hil, max(sizes), 9)
    _, wf64 = gr.f64_copy(wf)
    with torch.no_grad():
        _, margin = gr.log_psi_and_kink_margin(wf64, tp._states(hil, keys))
    return {m: int((margin[:m] < TAU).sum()) for m in sizes}


@pytest.mark.parametrize("shape,name", BACKWARD)
def test_backward_against_float64(shape, name):
    import test_pairs_gpu as tp
    kinks = _kink_rows(shape, name)
    assert all(k <= KINK_CAP * m for m, k in kinks.items()), kinks
    hil, wf = _case_net(shape, name)
    assert wf.fused() is not None and wf.fused().train_mode == "hip"         # (no shape is refused or handed to another path)
    tp._check_backward(f"{list(SHAPES[shape][0])} {name}", hil, wf)


def test_forward_after_library_training_steps(tmp_path):
    """test_pairs_gpu's trained-network check at a [16, 16] MLP on LiH: 50 steps of the library loop re-pack the phase layers
    inside every step; then the whole space against the float64 copy of the trained parameters."""
    import test_pairs_gpu as tp
    from naqs_amd.optimizer import PartialSamplingOptimizer
    from test_optimizer import ADAM
    tp._threads()
    hil, wf = _case_net("16x2", "LiH")
    _, N, na, nb, _ = gr.sector("LiH")
    opt = PartialSamplingOptimizer(
        n_samples=100000, n_samples_max=1e12, n_unq_samples_min=2, n_unq_samples_max=1e5, log_exact_energy=False, wavefunction=wf,
        qubit_hamiltonian=tp._row_ham("LiH", None), pre_compute_H=False, n_electrons=na + nb, n_alpha_electrons=na,
        n_beta_electrons=nb, normalise_psi=True, grad_clip_factor=None, optimizer=torch.optim.Adam,
        optimizer_args=[dict(a) for a in ADAM], save_loc=str(tmp_path), pauli_hamiltonian_dtype=np.float64, seed=5)
    assert opt._can_onecall() and opt._can_run_in_library()
    p0 = wf.flatten_parameters().clone()
    opt.run(n_epochs=50, save_freq=None, save_final=False, output_freq=10 ** 9)
    torch.cuda.synchronize()
    fused = wf._fused                                      # (not wf.fused(): no refresh from the version counters)
    assert fused is not None and fused is not False
    p1 = wf.flatten_parameters()
    assert bool(torch.isfinite(p1).all())
    moved = (p1 != p0).float().mean().item()
    assert moved > 0.5, moved
    _, wf64 = gr.f64_copy(wf)
    keys = np.sort(hil._all_keys()).astype(np.uint64)
    want = gr.log_psi_f64(wf64, tp._states(hil, keys))
    assert np.isfinite(want).all()
    lp = fused.log_psi(tp._kdev(keys))
    ran = fused.last_kernel()
    bad, e0, e1, r = _compare(lp.cpu().numpy(), want, hil.N // 2, np.abs(want[:, 1]).max(), 2)
    print(f"[trained [16, 16] LiH] 50 library steps, {100 * moved:.0f} % of the parameters moved  M={len(keys)} {ran}  |HIP - f64| log "
          f"{e0:.2e} phase {e1:.2e} ({r:.2f} x bound)")
    assert "phase_kernel_h" in ran, ran
    assert not bad, bad
