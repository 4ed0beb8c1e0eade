"""The training backward on the MI355X against float64 (tests/grad_reference.py), at every size class it dispatches on.

(a) the reference's own gradients through both call forms of the training step (the one-call naqs_net_train_backward_vmc
    of _SGD_step, and naqs_vmc_loss_grad + naqs_net_train_backward): magnitudes, not just the sign pattern one Adam step
    pins (test_sgd_step_matches_reference_step_on_device);
(b) naqs_vmc_loss_grad / _ev against their formula (energy.py:328-329, 372-375);
(c) forward_saved + backward_saved and backward_from_local_energy at the row counts where naqs_phase_grad.hip changes path
    (W0_FUSE_MAX_ROWS, SUMS_FUSE_MAX_ROWS, the grad_in tile height, the number of grad_w slices, 32 / 128-row tiles), per
    parameter tensor within 2e-5 of its scale of the float64 gradient.  Rows whose float64 ReLU inputs lie within TAU of
    zero (a float32 forward may take the other branch there) get g = 0 (w = 0 in the E_loc form).  Each case prints the
    HIP error and the error of float32 autograd on the CPU against the same float64 gradient.
"""
import os
import re

import numpy as np
import pytest

import grad_reference as gr
from conftest import GOLDEN, ROOT, golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TAU = 1e-5              # kink margin (float64 pre-activation) below which a row is left out
BOUND = 2e-5            # max |G_hip - G_f64| per tensor, in units of max |G_f64|


def _src_const(name):
    src = open(os.path.join(ROOT, "naqs-for-quantum-chemistry_amd", "csrc", "naqs_phase_grad.hip")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))


W0_FUSE = _src_const("W0_FUSE_MAX_ROWS")
SUMS_FUSE = _src_const("SUMS_FUSE_MAX_ROWS")
TB = _src_const("TB")


def _gin_switch(k1):
    """Largest M whose grad_in tiles are 32 rows high: ceil(M / 32) * (pad64(K1) / TB) <= 4 * CUs (naqs_phase_grad.hip)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    kp = (k1 + 63) // 64 * 64
    return 32 * (4 * cus // (kp // TB))


def _rel_err(got, want):
    scale = np.abs(want).max()
    d = np.abs(np.asarray(got, np.float64) - want).max()
    return d / scale if scale > 0 else (0.0 if d == 0 else np.inf)


def _dev_wf(fix):
    from test_nade import make_wf
    from test_variants import split
    try:
        mol = split(fix)[0]
    except ValueError:
        mol = fix
    hil, wf = make_wf(mol, golden(f"nade_{fix}.npz"), device="cuda")
    return mol, hil, wf


def _grads(wf):
    return {n: p.grad.detach().double().cpu().numpy().copy() for n, p in wf.model.named_parameters()}


def _zero_grad(wf):
    for p in wf.model.parameters():
        p.grad = None


def _sums(e, w):
    """(sum w Re E, sum w Im E, sum w Re(E)^2, sum w) (naqs_reduce.hpp), float64."""
    return np.array([(w * e.real).sum(), (w * e.imag).sum(), (w * e.real ** 2).sum(), w.sum()])


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _c2(e):
    return np.stack([e.real, e.imag], -1)


# ---------------------------------------------------------------------------------------------------------------- (a)
FUSED_ALL = ["LiH", "H2O", "N2", "LiH_noampsym", "LiH_fullmask", "N2_noampsym", "N2_nomask", "N2_0.75_fullmask", "N2_2.25_fullmask",
             "LiH_aggphase", "N2_aggphase", "LiH_phasesym", "LiH_phasesym_agg", "CH2_noampsym", "CH2_fullmask_noampsym",
             "LiH_qo1"]


def test_fused_list_covers_the_variant_suite():
    from test_variants_gpu import FUSED
    assert set(FUSED) <= set(FUSED_ALL)


@pytest.mark.parametrize("fix", FUSED_ALL)
def test_training_step_gradients_match_reference(fix):
    """The reference's _SGD_step gradients (grad:*) from its sampled table and E_loc, through both call forms; the pair
    (<E>, Var) of the same launch; the two forms bit for bit."""
    z = golden(f"nade_{fix}.npz")
    mol, hil, wf = _dev_wf(fix)
    fused = wf.fused()
    assert fused is not None and fused.train_mode == "hip"
    keys = _dev(z["samp_keys"].astype(np.int64), torch.int64)
    w = z["samp_counts"].astype(np.float64)
    w /= w.sum()
    e = z["sgd_eloc_c128"]
    e_d, w_d, sums_d = _dev(_c2(e)), _dev(w), _dev(_sums(e, w))

    _zero_grad(wf)
    _, saved = fused.forward_saved(keys)
    g1, ev1 = fused.backward_from_local_energy(saved, e_d, w_d, sums_d)
    grads1 = _grads(wf)
    _zero_grad(wf)
    fused._grad_flat = None
    _, saved = fused.forward_saved(keys)
    g2, ev2 = fused.vmc_loss_grad(e_d, w_d, sums_d, with_energy=True)
    fused.backward_saved(saved, g2)
    grads2 = _grads(wf)
    torch.cuda.synchronize()
    assert torch.equal(g1, g2) and torch.equal(ev1, ev2)
    E, var = ev1.cpu().numpy()
    assert abs(E - float(z["sgd_E"])) < 2e-5 * max(1, abs(E))
    assert abs(var - float(z["sgd_Var"])) < 1e-3 * max(1, abs(var))
    for name, p in wf.model.named_parameters():
        assert np.array_equal(grads1[name], grads2[name]), name
        g_ref = z["grad:" + name]
        scale = max(1e-3, np.abs(g_ref).max())
        assert np.max(np.abs(grads1[name] - g_ref)) < 2e-3 * scale, (name, np.max(np.abs(grads1[name] - g_ref)) / scale)


# ---------------------------------------------------------------------------------------------------------------- (b)
def _loss_grad_case(M, skew, seed=11):
    """N2-like local energies (-107.4 +- 0.5, imaginary parts ~1e-3) and skewed (log-normal) or uniform weights."""
    rs = np.random.RandomState(seed + M)
    e = rs.normal(-107.4, 0.5, M) + 1j * rs.normal(0.0, 1e-3, M)
    w = np.exp(rs.normal(0.0, 2.0, M)) if skew else np.ones(M)
    return e, w / max(w.sum(), 1e-300)


@pytest.mark.parametrize("M", [1, 255, 256, 257, 10003])
@pytest.mark.parametrize("skew", [True, False])
def test_loss_grad_kernel_matches_its_formula(M, skew):
    """g = (2 w Re(E - <E>), -2 w Im(E - <E>)) in float32:
    * bit for bit the documented arithmetic ((float)E - (float)sums[0]) * 2 (float)w;
    * within the float32 rounding bound of the float64 formula.  With u = 2^-24, fl(E) = E (1 + d1), fl(<E>) = <E> (1 + d2),
      the difference, 2 fl(w) (exact doubling) and the product each rounded once:
        |g32 - g64| <= 2 w [ (|E| + |<E>|) u + |E - <E>| 3 u ] (1 + 4 u)
      — the first term, the rounding of |E| ~ 107 before the cancellation, dominates;
    * (<E>, Var) = (sums[0] / sums[3], sums[2] / sums[3] - <E>^2) as float64, equal to the two-pass float64 formula to 1e-12 of
      the quantities they are formed from."""
    from naqs_amd import _lib
    from naqs_amd.hamiltonian import _stream_ptr
    lib = _lib.load_library()
    dev = torch.device("cuda:0")
    e, w = _loss_grad_case(M, skew)
    sums = _sums(e, w)
    e_d, w_d, sums_d = _dev(_c2(e)), _dev(w), _dev(sums)
    g = torch.full((M, 2), float("nan"), dtype=torch.float32, device=dev)
    ev = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    _lib.check(lib.naqs_vmc_loss_grad(M, e_d.data_ptr(), w_d.data_ptr(), sums_d.data_ptr(), g.data_ptr(), _stream_ptr(dev)),
               "naqs_vmc_loss_grad")
    g_plain = g.clone()
    _lib.check(lib.naqs_vmc_loss_grad_ev(M, e_d.data_ptr(), w_d.data_ptr(), sums_d.data_ptr(), g.data_ptr(), ev.data_ptr(),
                                         _stream_ptr(dev)), "naqs_vmc_loss_grad_ev")
    torch.cuda.synchronize()
    g, g_plain, ev = g.cpu().numpy(), g_plain.cpu().numpy(), ev.cpu().numpy()
    assert np.array_equal(g, g_plain)
    emu = gr.loss_grad_f32_emulated(e, w, sums)
    assert np.array_equal(g, emu), np.abs(g - emu).max()
    g64 = gr.loss_grad_f64(e, w)
    mean = (w * e).sum()
    u = 2.0 ** -24
    bound = 2 * w * ((np.abs(e.real) + abs(mean.real)) * u + np.abs(e.real - mean.real) * 3 * u) * (1 + 4 * u)
    bound_im = 2 * w * ((np.abs(e.imag) + abs(mean.imag)) * u + np.abs(e.imag - mean.imag) * 3 * u) * (1 + 4 * u)
    # (+ the float64 rounding of sums[0] against the formula's own <E>: ~1e-16 relative)
    assert np.all(np.abs(g[:, 0] - g64[:, 0]) <= bound + 1e-15 * 2 * w * abs(mean))
    assert np.all(np.abs(g[:, 1] - g64[:, 1]) <= bound_im + 1e-15 * 2 * w * abs(mean))
    E = mean.real / w.sum()
    var = (w * (e.real - E) ** 2).sum() / w.sum()
    assert abs(ev[0] - E) <= 1e-12 * abs(E)
    assert abs(ev[1] - var) <= 1e-12 * (sums[2] / sums[3])
    assert np.array_equal(ev, [sums[0] / sums[3], sums[2] / sums[3] - (sums[0] / sums[3]) ** 2])


def test_loss_grad_kernel_energy_of_an_empty_table():
    from naqs_amd import _lib
    from naqs_amd.hamiltonian import _stream_ptr
    lib = _lib.load_library()
    dev = torch.device("cuda:0")
    sums = np.array([-107.25, 0.001, 11502.9, 1.0])
    sums_d = _dev(sums)
    ev = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    _lib.check(lib.naqs_vmc_loss_grad_ev(0, None, None, sums_d.data_ptr(), None, ev.data_ptr(), _stream_ptr(dev)),
               "naqs_vmc_loss_grad_ev")
    _lib.check(lib.naqs_vmc_loss_grad(0, None, None, sums_d.data_ptr(), None, _stream_ptr(dev)), "naqs_vmc_loss_grad")
    torch.cuda.synchronize()
    assert np.array_equal(ev.cpu().numpy(), [sums[0] / sums[3], sums[2] / sums[3] - (sums[0] / sums[3]) ** 2])


# ---------------------------------------------------------------------------------------------------------------- (c)
def _random_net(phase_hidden):
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    torch.manual_seed(3)
    hil = Hilbert.get(30, 7, 7, encoding=Encoding.SIGNED)
    wf = NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, amp_hidden_size=[64], phase_hidden_size=phase_hidden,
                                   use_amp_spin_sym=True, use_phase_spin_sym=False, aggregate_phase=False,
                                   n_alpha_electrons=7, n_beta_electrons=7)
    return "Li2O", hil, wf


def _random_keys(hil, M, seed):
    """M distinct physical keys of the sector (the 30-qubit 7 + 7 space here), in random order."""
    return gr.random_keys(hil, M, seed)


def _whole_space(hil, seed):
    return np.random.RandomState(seed).permutation(hil.restricted2full_idx(np.arange(hil.size)).astype(np.uint64))


# family: (network, key set, cuts of the backward_saved form, cuts of the E_loc form, environment / mode)
def _families():
    return {
        "N2": ("N2", None, lambda sw: [1, 2, 31, 32, 33, 127, 128, 129, W0_FUSE - 1, W0_FUSE, W0_FUSE + 1, SUMS_FUSE + 1,
                                       sw(512) - 1, sw(512), sw(512) + 1, 10000, 14400], [33, 4097, 10000], {}),
        "N2_mega0": ("N2", None, lambda sw: [33, W0_FUSE + 1, 10000], [33, 10000], {"NAQS_TRAIN_MEGA": "0"}),
        "N2_blas": ("N2", None, lambda sw: [33, W0_FUSE + 1, 10000], [], {"mode": "blas"}),
        "N2_noampsym": ("N2_noampsym", None, lambda sw: [129, W0_FUSE + 1, 10000], [10000], {}),
        "N2_nomask": ("N2_nomask", None, lambda sw: [129, W0_FUSE + 1, 10000], [10000], {}),
        "N2_2.25_fullmask": ("N2_2.25_fullmask", None, lambda sw: [129, W0_FUSE + 1, 10000], [10000], {}),
        "N2_aggphase": ("N2_aggphase", None, lambda sw: [1, 127, 128, 129, W0_FUSE + 1, 14400], [129, 14400], {}),
        "LiH_phasesym": ("LiH_phasesym", None, lambda sw: [1, 33, 225], [225], {}),
        "LiH_phasesym_agg": ("LiH_phasesym_agg", None, lambda sw: [1, 33, 225], [225], {}),
        "CH2_noampsym": ("CH2_noampsym", None, lambda sw: [1, 33, 735], [735], {}),
        "rand30_512": ("rand", [512, 512], lambda sw: [W0_FUSE + 1, 50000], [50000], {}),
        "rand30_64": ("rand", [64, 64], lambda sw: [sw(64) - 1, sw(64), sw(64) + 1], [], {}),
    }


def _segment_grads(wf, states, g, cuts, tau=None):
    """Cumulative sums over rows [0, cut) of d/d theta g . log psi for every cut, each row evaluated once (one forward per
    segment between consecutive cuts) -> ({cut: {name: grad}}, kink margin [max cut]).  With ``tau`` the rows of g whose
    margin is below it are zeroed in place before their backward pass."""
    out, acc, margins, lo = {}, None, [], 0
    for hi in sorted(set(cuts)):
        lp, margin = gr.log_psi_and_kink_margin(wf, states[lo:hi])
        margins.append(margin)
        if tau is not None:
            g[lo:hi] = gr.kink_free(g[lo:hi], margin, tau)[0]
        gseg = gr.grad_f64(wf, None, g[lo:hi], lp=lp)
        acc = gseg if acc is None else {k: acc[k] + gseg[k] for k in acc}
        out[hi] = {k: v.copy() for k, v in acc.items()}
        lo = hi
    return out, np.concatenate(margins)


@pytest.mark.parametrize("family", list(_families()))
def test_backward_against_float64_at_every_size_class(family, monkeypatch):
    from naqs_amd import hamiltonian, packing
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    src, phase_hidden, cuts_fn, eloc_cuts, env = _families()[family]
    for k, v in env.items():
        if k != "mode":
            monkeypatch.setenv(k, v)
    if src == "rand":
        mol, hil, wf = _random_net(phase_hidden)
    else:
        mol, hil, wf = _dev_wf(src)
    fused = wf.fused()
    assert fused is not None
    if env.get("mode"):
        fused.train_mode = env["mode"]
    cuts = sorted(set(cuts_fn(_gin_switch)))
    _, wf64 = gr.f64_copy(wf)
    _, wf32 = gr.f64_copy(wf, dtype=torch.float32)
    M = max(cuts + eloc_cuts)
    keys = _random_keys(hil, M, 5) if src == "rand" else _whole_space(hil, 5)[:M]
    assert len(keys) == M, (family, len(keys), M)
    states = hil.idx2state(torch.as_tensor(keys.astype(np.int64)))
    rs = np.random.RandomState(7)
    g = rs.normal(size=(M, 2)).astype(np.float32).astype(np.float64) / np.sqrt(M)

    # the float64 gradient of every prefix (and, from the same forward passes, the margins that zero g's kink rows), then
    # float32 autograd on the CPU with the same g
    ref64, margin = _segment_grads(wf64, states, g, cuts + eloc_cuts, tau=TAU)
    n_kink = int((margin < TAU).sum())
    assert n_kink <= 0.1 * M, (family, n_kink, M)
    ref32, _ = _segment_grads(wf32, states, g.astype(np.float32), cuts + eloc_cuts)

    fails = []
    for m in cuts:
        order = np.argsort(keys[:m])
        k_d = _dev(keys[:m][order].astype(np.int64), torch.int64)
        _zero_grad(wf)
        _, saved = fused.forward_saved(k_d)
        fused.backward_saved(saved, _dev(g[:m][order], torch.float32))
        got = _grads(wf)
        e_hip = max(_rel_err(got[n], ref64[m][n]) for n in got)
        e_f32 = max(_rel_err(ref32[m][n], ref64[m][n]) for n in got)
        print(f"[backward {family} {fused.train_mode}] M={m:6d} kink rows zeroed {int((margin[:m] < TAU).sum()):5d} "
              f"({(margin[:m] < TAU).mean():.1%})  |HIP - f64| {e_hip:.2e}  |torch f32 CPU - f64| {e_f32:.2e}")
        fails += [(m, n, _rel_err(got[n], ref64[m][n])) for n in got if not _rel_err(got[n], ref64[m][n]) <= BOUND]

    if eloc_cuts:
        ham = hamiltonian.DevicePauliHamiltonian(packing.load_packed(os.path.join(GOLDEN, f"ham_{mol}.npz")), device="cuda:0")
        for m in eloc_cuts:
            order = np.argsort(keys[:m])
            ks, near = keys[:m][order], (margin[:m] < TAU)[order]
            w = rs.uniform(0.5, 1.5, m)
            w[near] = 0.0
            w /= w.sum()
            k_d = _dev(ks.astype(np.int64), torch.int64)
            _zero_grad(wf)
            fused._grad_flat = None
            _, saved, eloc, sums = fused.forward_saved_with_local_energy(ham, k_d, _dev(w))
            g_k, ev = fused.backward_from_local_energy(saved, eloc, _dev(w), sums)
            got = _grads(wf)
            e = eloc.cpu().numpy()
            e = e[:, 0] + 1j * e[:, 1]
            assert np.all(np.isfinite(e))
            g64 = gr.loss_grad_f64(e, w)
            st = states[torch.as_tensor(order)]
            want = gr.grad_f64(wf64, st, g64)
            want32 = gr.grad_f64(wf32, st, g64.astype(np.float32))
            e_hip = max(_rel_err(got[n], want[n]) for n in got)
            e_f32 = max(_rel_err(want32[n], want[n]) for n in got)
            print(f"[backward+E_loc {family}] M={m:6d} kink rows zeroed {int(near.sum()):5d}  <E> {ev[0].item():.6f}  "
                  f"|HIP - f64| {e_hip:.2e}  |torch f32 CPU - f64| {e_f32:.2e}")
            E = (w * e.real).sum()
            assert abs(ev[0].item() - E) < 1e-9 * abs(E)
            fails += [("eloc", m, n, _rel_err(got[n], want[n])) for n in got if not _rel_err(got[n], want[n]) <= BOUND]
    assert not fails, fails
