"""The float64 reference of the training backward (tests/grad_reference.py) pinned to the reference's own vectors: a float64
copy of every ``nade_*.npz`` network reproduces the recorded loss and gradients of _SGD_step, and float32 networks are
untouched by the modules following their parameters' dtype.  test_backward_gpu.py holds the HIP backward to this reference,
test_forward_f64_gpu.py the HIP forward and the sampler's probabilities."""
import glob
import os

import numpy as np
import pytest
import torch

import grad_reference as gr
from conftest import GOLDEN, golden

FIXTURES = sorted(os.path.basename(f)[5:-4] for f in glob.glob(os.path.join(GOLDEN, "nade_*.npz")))


def test_every_fixture_is_listed():
    assert len(FIXTURES) == 17 and "N2" in FIXTURES and "CH2_noampsym" in FIXTURES and "LiH_qo1" in FIXTURES


@pytest.mark.parametrize("fix", FIXTURES)
def test_f64_modules_reproduce_reference_loss_and_gradients(fix):
    """loss = 2 Re sum_i w_i log psi_i (E_i - <E>)^* on the reference's sampled states with its E_loc (energy.py:328-329),
    autograd in float64: the recorded sgd_loss and grad:* to 2e-3 of each tensor's scale (the reference ran in float32)."""
    z = golden(f"nade_{fix}.npz")
    hil, wf = gr.f64_copy(fix)
    assert all(p.dtype == torch.float64 for p in wf.model.parameters())
    s = torch.tensor(z["samp_states"])
    lp, margin = gr.log_psi_and_kink_margin(wf, s)
    assert lp.dtype == torch.float64 and margin.shape == (len(s),) and np.all(margin >= 0)
    assert np.max(np.abs(lp.detach().numpy() - z["samp_log_psi"])) < 5e-5
    w = z["samp_counts"].astype(np.float64)
    w /= w.sum()
    e = z["sgd_eloc_c128"]
    d = e - (w * e).sum()
    loss = 2 * (torch.as_tensor(w) * (lp[:, 0] * torch.as_tensor(d.real) - lp[:, 1] * torch.as_tensor(d.imag))).sum()
    assert abs(loss.item() - float(z["sgd_loss"])) < 1e-4 * max(1, abs(float(z["sgd_loss"])))
    got = gr.grad_f64(wf, s, gr.loss_grad_f64(e, w), lp=lp)
    for name, p in wf.model.named_parameters():
        g_ref = z["grad:" + name]
        scale = max(1e-3, np.abs(g_ref).max())
        assert np.max(np.abs(got[name] - g_ref)) < 2e-3 * scale, (name, np.max(np.abs(got[name] - g_ref)) / scale)


def test_float32_networks_are_unchanged():
    """The float32 copy built by f64_copy(dtype=float32) and the fixture's own float32 network give the same bits."""
    from test_nade import make_wf
    z = golden("nade_N2.npz")
    _, wf = make_wf("N2", z)
    _, wf32 = gr.f64_copy(wf, dtype=torch.float32)
    s = torch.tensor(z["samp_states"][:500])
    with torch.no_grad():
        a = wf.log_psi(s)
        b = wf32.log_psi(s)
    assert a.dtype == torch.float32 and torch.equal(a, b)


def test_loss_gradient_helpers():
    rs = np.random.RandomState(0)
    M = 1000
    e = rs.normal(-107.4, 0.5, M) + 1j * rs.normal(0, 1e-3, M)
    w = rs.uniform(0.5, 1.5, M)
    w /= w.sum()
    g64 = gr.loss_grad_f64(e, w)
    sums = np.array([(w * e.real).sum(), (w * e.imag).sum(), (w * e.real ** 2).sum(), w.sum()])
    g32 = gr.loss_grad_f32_emulated(e, w, sums)
    assert g32.dtype == np.float32
    assert np.max(np.abs(g32 - g64)) < 1e-7 and np.max(np.abs(g64)) > 1e-4
    assert abs(g64[:, 0].sum()) < 1e-12                             # sum_i w_i (E_i - <E>) = 0
    g, n = gr.kink_free(g64, np.r_[np.zeros(3), np.ones(M - 3)])
    assert n == 3 and not g[:3].any() and np.array_equal(g[3:], g64[3:])


def test_kink_margin_sees_every_relu():
    """The margin is the smallest |ReLU input| over the amplitude blocks (torch.relu) AND the phase MLP (nn.ReLU)."""
    relu = torch.relu
    hil, wf = gr.f64_copy("N2")
    s = torch.tensor(golden("nade_N2.npz")["samp_states"][:64])
    lp, margin = gr.log_psi_and_kink_margin(wf, s)
    phase0 = wf.model.phase_layers[0].layers[0][0]                # nn.Linear -> nn.ReLU of the phase MLP
    amp0 = wf.model.amp_layers[0].layers[0][0]                      # block 0 sees a zero input: its pre-activation is its bias
    with torch.no_grad():
        b_ph, b_amp = phase0.bias.clone(), amp0.bias.clone()
        # a phase unit whose pre-activation is exactly zero for row 0: that row's margin drops to 0
        x = s[:1].to(torch.float64)[..., wf._q2m]
        P = wf.model.P
        xin = torch.cat([x[:, 0:2 * (P - 1):2], x[:, 1:2 * (P - 1):2]], -1)
        phase0.bias[0] = -(xin @ phase0.weight[0])[0]
        _, m_ph = gr.log_psi_and_kink_margin(wf, s)
        phase0.bias.copy_(b_ph)
        amp0.bias[3] = 0.0                                          # a zero pre-activation in every row (torch.relu)
        _, m_amp = gr.log_psi_and_kink_margin(wf, s)
        amp0.bias.copy_(b_amp)
    assert m_ph[0] < 1e-12 < margin[0] and np.all(margin > 0)
    assert np.all(m_amp == 0)
    assert torch.relu is relu                                       # (the wrapper is gone again)


@pytest.mark.parametrize("fix", FIXTURES)
def test_f64_forward_reproduces_reference_log_psi(fix):
    """log_psi_f64 (chunked, float64) of the reference's eval_states against its recorded float32 eval_log_psi: the recorded
    values differ from float64 by float32 rounding only, within the bounds test_forward_f64_gpu.py holds the HIP forward to
    (log|psi|: 2e-6 + 2e-7 |log|psi||, measured <= 1.3e-6; phase: 5e-6 max |phase|, measured <= 5.3e-7).  Chunks of 7 rows
    give one pass's numbers to float64 rounding (the GEMMs block differently)."""
    z = golden(f"nade_{fix}.npz")
    hil, wf = gr.f64_copy(fix)
    s = torch.tensor(z["eval_states"])
    lp = gr.log_psi_f64(wf, s)
    assert lp.dtype == np.float64 and lp.shape == (len(s), 2)
    assert np.max(np.abs(gr.log_psi_f64(wf, s, chunk=7) - lp)) < 1e-12
    ref = z["eval_log_psi"].astype(np.float64)
    assert np.array_equal(np.isfinite(lp), np.isfinite(ref))
    fin = np.isfinite(ref[:, 0])
    d = np.abs(lp - ref)
    assert np.all(d[fin, 0] <= 2e-6 + 2e-7 * np.abs(ref[fin, 0])), d[fin, 0].max()
    assert np.all(d[:, 1] <= 5e-6 * max(1e-3, np.abs(lp[:, 1]).max())), d[:, 1].max()


def test_sorted_rows():
    keys = np.array([9, 3, 7, 1, 5], np.uint64)
    t = np.arange(10.0).reshape(5, 2)
    k, r = gr.sorted_rows(keys, 4, t)
    assert k.tolist() == [1, 3, 7, 9] and r[:, 0].tolist() == [6, 2, 4, 0]


@pytest.mark.parametrize("fix", ["N2", "N2_nomask", "N2_aggphase", "LiH_fullmask", "LiH_phasesym_agg"])
def test_sampler_probs_are_psi_squared_in_float64(fix):
    """The identity test_forward_f64_gpu.py's sampler check rests on: the probs of the torch sampler (_forward_sample: the
    product over pairs of the conditional |amplitude|^2, nade.py:351-365) are exp(2 log|psi|) of the drawn states — with
    PARTIAL, NONE and FULL masking and the aggregate phase — to float64 rounding."""
    hil, wf = gr.f64_copy(fix)
    states, counts, probs = wf.sample(100000, ret_log_psi=False, use_fused=False, generator=torch.Generator().manual_seed(5))
    assert probs.dtype == torch.float64 and len(probs) > 200 and counts.sum() > 0
    want = np.exp(2 * gr.log_psi_f64(wf, states)[:, 0])
    assert np.max(np.abs(probs.numpy() / want - 1)) < 1e-13


# ------------------------------------------------------------------------------- the orbital-pair sectors (test_pairs_gpu.py)
def test_sector_table_matches_the_packed_molecules():
    """One sector per P = 2..16 (P = 10 four times: the extreme fillings); a molecule's row is its qubit count and the
    electron split system.Molecule gives packing_terms.npz's electrons and multiplicity (as test_packing.py packs them)."""
    import math
    from naqs_amd import system
    z = np.load(os.path.join(GOLDEN, "packing_terms.npz"))
    assert sorted({r[1] // 2 for r in gr.SECTORS}) == list(range(2, 17))
    assert sorted(r[1] for r in gr.SECTORS if r[1] == 20) == [20] * 4
    for name, N, na, nb, mol in gr.SECTORS:
        assert N % 2 == 0 and 1 <= na <= N // 2 and 1 <= nb <= N // 2, name
        if mol is None:
            continue
        m = object.__new__(system.Molecule)
        m.n_electrons, m.multiplicity = (int(v) for v in z[f"{mol}:electrons"])
        assert (z[f"{mol}:ops"].shape[1], m.get_n_alpha_electrons(), m.get_n_beta_electrons()) == (N, na, nb), name
    sizes = {name: math.comb(N // 2, na) * math.comb(N // 2, nb) for name, N, na, nb, _ in gr.SECTORS}
    assert (sizes["H2"], sizes["syn6_2_1"], sizes["H2_6-31G"], sizes["syn10_3_2"], sizes["H2_cc-pvdz"], sizes["F2"],
            sizes["O2"], sizes["H2O_6-31G"], sizes["LiCl"]) == (4, 9, 16, 100, 100, 100, 1200, 1656369, 1002001)


def test_random_keys_of_any_sector():
    from naqs_amd.hilbert import Hilbert
    for N, na, nb, M in ((4, 1, 1, 4), (6, 2, 1, 9), (20, 9, 7, 500), (32, 8, 8, 2000)):
        hil = Hilbert.get(N, na, nb)
        k = gr.random_keys(hil, M, 3)
        assert len(k) == M and len(np.unique(k)) == M and hil.is_physical(k).all()
        assert np.array_equal(k, gr.random_keys(hil, M, 3))
    assert (gr.random_keys(Hilbert.get(32, 8, 8), 2000, 3) >> np.uint64(31)).any()        # (bit 31: beta orbital 15)


@pytest.mark.parametrize("fix", ["LiH", "H2O", "LiH_fullmask", "LiH_noampsym"])
def test_log_amp_is_log_psi_without_the_phase(fix):
    """log_amp_f64 (the sampler's per-block conditionals) equals log_psi_f64[:, 0] (the teacher-forced forward) on the whole
    space — and -inf where the forward has -inf (FULL masking, unphysical keys)."""
    from naqs_amd.hilbert import Hilbert
    hil, wf = gr.f64_copy(fix)
    keys = np.sort(hil._all_keys()).astype(np.uint64)
    if fix.endswith("fullmask"):
        full = Hilbert.get(hil.N, hil.N_alpha, hil.N_beta)
        extra = np.setdiff1d(np.arange(1 << hil.N, dtype=np.uint64)[::7], keys)[:300]
        assert not full.is_physical(extra).any()
        keys = np.concatenate([keys, extra])
    s = hil.idx2state(torch.as_tensor(keys.astype(np.int64)))
    a = gr.log_amp_f64(wf, s, chunk=97)
    b = gr.log_psi_f64(wf, s)[:, 0]
    assert np.array_equal(np.isfinite(a), np.isfinite(b))
    if fix.endswith("fullmask"):
        assert (~np.isfinite(a)).sum() >= 250
    f = np.isfinite(b)
    assert np.max(np.abs(a[f] - b[f])) < 1e-12


@pytest.mark.parametrize("masking", ["PARTIAL", "FULL"])
def test_conditionals_multiply_to_psi_squared(masking):
    """LiH: the product of conditionals_f64 along each key's path is exp(2 log|psi|); under masking the conditionals of
    every node sum to one over the physical outcomes, which alone carry mass (PARTIAL: except the last pair)."""
    from naqs_amd.nade import NadeMasking
    from test_nade import make_wf
    hil, wf = make_wf("LiH", golden("nade_LiH.npz"), masking=NadeMasking[masking])
    _, wf = gr.f64_copy(wf)
    keys = np.sort(hil._all_keys())
    s = hil.idx2state(torch.as_tensor(keys))
    ms = s[:, wf._q2m]
    occ = ((ms[:, 0::2] > 0).long() + 2 * (ms[:, 1::2] > 0).long()).numpy()
    prod = np.ones(len(keys))
    for n in range(wf.model.P):
        p, phys = gr.conditionals_f64(wf, s, n)
        assert p.shape == (len(keys), 4) and phys.shape == (len(keys), 4)
        if masking == "FULL" or n < wf.model.P - 1:
            assert np.all(p[~phys] == 0) and np.allclose(p.sum(1), 1, rtol=0, atol=1e-14)
        prod *= p[np.arange(len(keys)), occ[:, n]]
    want = np.exp(2 * gr.log_psi_f64(wf, s)[:, 0])
    assert np.max(np.abs(prod / want - 1)) < 1e-12
