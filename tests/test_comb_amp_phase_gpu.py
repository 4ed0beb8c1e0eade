"""Combined amplitude-phase blocks with a single phase (``-single_phase -comb_amp_phase``; naqs_net_create_combined) on the MI355X.

* the handle: the reference's fixtures (tests/golden/comb_*.npz: LiH with and without the spin symmetry, N2) and the N2 published
  widths get a combined handle, no fallback notice; log psi of the fixtures within 5e-5 of the reference's; naqs_logpsi_eloc the
  same bits as naqs_net_logpsi and the E_loc of ham.local_energy;
* log psi against the float64 copy of the network (tests/grad_reference.py) at every P = 2..16 (grad_reference.SECTORS), both
  symmetry settings: PARTIAL masking at every P, FULL and NONE at P = 2, 5, 10, 16; amplitude widths 16, 64, 128; M = 1, 63, 64,
  10^4 (at most the sector's size).  Bounds of test_forward_f64_gpu.py (_compare).  The training forward gives the same bits;
* the sampler: the draw (keys, counts, probs) bit for bit that of a naqs_net_create handle with the same amplitude rows, probs
  against float64, an exact chi-square on LiH and H2O;
* gradients of both training-step call forms against float64 autograd (2e-5 of each tensor's scale; rows within 1e-5 of a ReLU
  kink get w = 0), bit for bit equal to each other, at M = 1, 64, 1000, 10^4; against the fixtures' grad:* (2e-3 of scale);
  naqs_net_amp_backward: log|psi| only, zero for the phase rows;
* naqs_vmc_run equal to step-by-step calls, bit for bit; the naqs_vmc_shard_* calls refuse combined handles;
* H2O trained with test_config3_gpu.py's flags plus -comb_amp_phase (10 000 steps, seed 111).
"""
import ctypes
import os

import numpy as np
import pytest

import grad_reference as gr
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TAU, GRAD_BOUND, U32 = 1e-5, 2e-5, 2.0 ** -24
FIXTURES = [("LiH", "LiH_single"), ("LiH", "LiH_nosym"), ("N2", "N2_single")]


def _threads():
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))


def _fixture(mol, fix):
    from test_nade import make_wf
    z = golden(f"comb_{fix}.npz")
    hil, wf = make_wf(mol, z, device="cuda")
    return z, hil, wf


def _net(name, sym=True, masking="PARTIAL", ha=64, seed=0, comb=True):
    """(hilbert, network) on sector `name` of grad_reference.SECTORS: -single_phase -comb_amp_phase with amplitude width `ha`
    (comb=False: the published single-phase ansatz of the same amplitude shape)."""
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.nade import NadeMasking
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    _, N, na, nb, _ = gr.sector(name)
    hil = Hilbert.get(N, na, nb, encoding=Encoding.SIGNED)
    torch.manual_seed(seed)
    wf = NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, masking=NadeMasking[masking], amp_hidden_size=[ha],
                                   phase_hidden_size=[64], use_amp_spin_sym=sym, use_phase_spin_sym=sym and comb,
                                   aggregate_phase=False, combined_amp_phase_blocks=comb, n_alpha_electrons=na, n_beta_electrons=nb)
    return hil, wf


def _states(hil, keys):
    return hil.idx2state(torch.as_tensor(np.asarray(keys).astype(np.int64)))


def _kdev(keys):
    return torch.as_tensor(np.asarray(keys).astype(np.int64), device="cuda")


def _amp_kernel(ha):
    return f"amp_mfma_kernel<{ha // 16}>" if ha in (32, 64, 128) else "amp_kernel"


def _expect(ha):
    return f"{_amp_kernel(ha)} + comb_head_kernel + comb_finish_kernel"


def _ham(mol):
    from naqs_amd import hamiltonian, packing
    return hamiltonian.DevicePauliHamiltonian(packing.load_packed(os.path.join(ROOT, "tests", "golden", f"ham_{mol}.npz")),
                                              device="cuda")


# --------------------------------------------------------------------------------------------------------------- handle
@pytest.mark.parametrize("mol,fix", FIXTURES)
def test_fixtures_get_a_combined_handle(mol, fix, capsys):
    z, hil, wf = _fixture(mol, fix)
    fused = wf.fused()
    assert fused is not None and fused.comb and fused.train_mode == "hip"
    assert "not available" not in capsys.readouterr().out
    n = sum(p.numel() for p in wf.model.parameters())
    assert fused.n_params == fused.n_amp_params == n
    kd = _kdev(z["eval_keys"])
    lp = fused.log_psi(kd)
    torch.cuda.synchronize()
    assert fused.last_kernel() == _expect(64)
    assert np.max(np.abs(lp.cpu().numpy() - z["eval_log_psi"])) < 5e-5
    # naqs_logpsi_eloc: the same log psi, the E_loc of ham.local_energy of that log psi
    ham = _ham(mol)
    keys = _kdev(np.sort(z["samp_keys"]))
    lp = fused.log_psi(keys)
    lp_e, e = fused.log_psi_and_local_energy(ham, keys)
    torch.cuda.synchronize()
    assert torch.equal(lp, lp_e)
    e_ref = ham.local_energy(keys, lp, kind="log_psi")
    assert torch.equal(e.reshape(e_ref.shape), e_ref)


@pytest.mark.parametrize("sym", [True, False])
def test_published_n2_widths_get_a_combined_handle(sym, capsys):
    hil, wf = _net("LiF", sym=sym)                     # (P = 10 like N2: the published -n_hid 64)
    fused = wf.fused()
    assert fused is not None and fused.comb and fused.amp_depth == 1
    assert "not available" not in capsys.readouterr().out
    n = ctypes.c_int64(0)
    assert fused._lib.naqs_net_param_count(fused._h, ctypes.byref(n)) == 0 and n.value == fused.n_params


def test_aggregate_and_deep_combined_blocks_stay_on_torch(capsys):
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    hil = Hilbert.get(12, 2, 2, encoding=Encoding.SIGNED)
    for agg, depth in ((True, 1), (False, 2)):
        wf = NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, amp_hidden_size=[32] * depth, phase_hidden_size=[32],
                                       aggregate_phase=agg, combined_amp_phase_blocks=True, n_alpha_electrons=2, n_beta_electrons=2)
        assert wf.fused() is None
        assert "fused HIP network kernels not available" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------------ forward vs f64
def _forward_cases():
    cases = []
    widths = [16, 64, 128]
    for i, row in enumerate(gr.SECTORS):
        for sym in (True, False):
            cases.append((row[0], sym, "PARTIAL", widths[(i + (0 if sym else 1)) % 3]))
    for name in ("H2", "syn10_3_2", "LiF", "syn32_8_8"):            # P = 2, 5, 10, 16
        for masking in ("FULL", "NONE"):
            for sym in (True, False):
                cases.append((name, sym, masking, 16 if name == "syn10_3_2" else (64 if sym else 128)))
    return cases


@pytest.mark.parametrize("name,sym,masking,ha", _forward_cases())
def test_forward_against_float64(name, sym, masking, ha):
    import test_forward_f64_gpu as tf
    _threads()
    hil, wf = _net(name, sym=sym, masking=masking, ha=ha, seed=3)
    fused = wf.fused()
    assert fused is not None and fused.comb
    ms = sorted({min(m, hil.size) for m in (1, 63, 64, 10000)})
    keys = gr.random_keys(hil, max(ms), seed=5)
    _, w64 = gr.f64_copy(wf)
    want = gr.log_psi_f64(w64, _states(hil, keys))
    P = hil.N // 2
    for M in ms:
        kd = _kdev(keys[:M])
        got = fused.log_psi(kd)
        torch.cuda.synchronize()
        assert fused.last_kernel() == _expect(ha), fused.last_kernel()
        bad, d0, d1, r = tf._compare(got.cpu().numpy(), want[:M], P)
        assert not bad, (name, sym, masking, ha, M, bad)
        lp2, _ = fused.forward_saved(kd)                  # the training forward: the same launches, the same bits
        torch.cuda.synchronize()
        assert torch.equal(lp2, got)


@pytest.mark.parametrize("name,sym", [("LiH", True), ("LiH", False), ("LiF", True), ("O2", False), ("syn32_8_8", True)])
def test_phase_rows_against_float64(name, sym):
    """The phase head with large, distinct phase biases (40, -25, 60, 15): the phase of a row is dominated by the bias of the row
    its outcome selects, so the bound (5e-6 of the table's largest |phase|) resolves a relative change of 2^-15 of one bias, a
    wrong row or a missing pi — and the amplitude rows are untouched by them."""
    import test_forward_f64_gpu as tf
    _threads()
    hil, wf = _net(name, sym=sym, seed=6)
    na, nph = (5, 3) if sym else (4, 4)
    last = wf.model.amp_layers[-1].linears()[1]
    with torch.no_grad():
        last.bias[na:] = torch.tensor([40.0, -25.0, 60.0, 15.0][:nph], device="cuda")
    fused = wf.fused()
    assert fused.comb
    keys = gr.random_keys(hil, min(hil.size, 4000), seed=2)
    _, w64 = gr.f64_copy(wf)
    want = gr.log_psi_f64(w64, _states(hil, keys))
    got = fused.log_psi(_kdev(keys)).cpu().numpy()
    bad, d0, d1, r = tf._compare(got, want, hil.N // 2)
    assert not bad, (name, sym, bad)
    # every phase row is selected by some row of the table
    assert len(np.unique(np.round(want[:, 1] / 5))) >= nph


# ---------------------------------------------------------------------------------------------------------------- sampler
def _plain_twin(wf, name, sym, ha):
    """A naqs_net_create network (single phase MLP) whose amplitude blocks are `wf`'s amplitude rows."""
    hil, plain = _net(name, sym=sym, ha=ha, comb=False, seed=9)
    na = 5 if sym else 4
    with torch.no_grad():
        for src, dst in zip(wf.model.amp_layers, plain.model.amp_layers):
            (a1, a2), (b1, b2) = src.linears(), dst.linears()
            b1.weight.copy_(a1.weight); b1.bias.copy_(a1.bias)
            b2.weight.copy_(a2.weight[:na]); b2.bias.copy_(a2.bias[:na])
    return plain


@pytest.mark.parametrize("name,sym,ha", [("H2", True, 64), ("syn10_3_2", False, 32), ("LiH", True, 64), ("LiH", False, 16),
                                         ("LiF", True, 64), ("O2", False, 128), ("Li2O", True, 64), ("syn32_8_8", False, 64)])
def test_sampler_draws_what_a_plain_handle_draws(name, sym, ha):
    hil, wf = _net(name, sym=sym, ha=ha, seed=4)
    plain = _plain_twin(wf, name, sym, ha)
    fc, fp = wf.fused(), plain.fused()
    assert fc.comb and not getattr(fp, "comb", False)
    for n, seed in ((1000, 1), (10 ** 5, 2), (10 ** 6, 3)):
        cap = 1 << 20
        a = fc.sample(n, seed=seed, max_unique=cap)
        b = fp.sample(n, seed=seed, max_unique=cap)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (name, n)
    # probs against float64: within 2 (log|psi| bound) + 8 P 2^-24 relative of exp(2 log|psi|_f64)
    import test_forward_f64_gpu as tf
    keys, counts, probs = a
    k = keys.cpu().numpy().astype(np.uint64)
    _, w64 = gr.f64_copy(wf)
    lp64 = gr.log_amp_f64(w64, _states(hil, k))
    P = hil.N // 2
    rel = np.abs(probs.double().cpu().numpy() / np.exp(2 * lp64) - 1)
    assert np.all(rel <= 2 * tf._bound_log(lp64, P) + 8 * P * U32), rel.max()
    # ... and log|psi| of the same keys is the sampler's target
    lp = fc.log_psi(keys)[:, 0].double().cpu().numpy()
    assert np.all(np.abs(lp - lp64) <= tf._bound_log(lp64, P))


@pytest.mark.parametrize("mol,sym", [("LiH", True), ("LiH", False), ("H2O", True)])
def test_sampler_exact_chi2(mol, sym):
    from scipy import stats
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    from test_nade import ELECTRONS
    N, na, nb = ELECTRONS[mol]
    hil = Hilbert.get(N, na, nb, encoding=Encoding.SIGNED, make_basis=True)
    torch.manual_seed(7)
    wf = NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, amp_hidden_size=[64], phase_hidden_size=[64],
                                   use_amp_spin_sym=sym, use_phase_spin_sym=sym, aggregate_phase=False,
                                   combined_amp_phase_blocks=True, n_alpha_electrons=na, n_beta_electrons=nb)
    fused = wf.fused()
    assert fused.comb
    n = 10 ** 8
    keys, counts, _ = fused.sample(n, seed=20240607, max_unique=hil.size + 16)
    k, c = keys.cpu().numpy().astype(np.uint64), counts.cpu().numpy()
    all_keys = np.sort(hil._all_keys()).astype(np.uint64)
    pos = np.searchsorted(all_keys, k)
    assert np.array_equal(all_keys[pos], k) and c.sum() <= n
    obs = np.zeros(len(all_keys))
    obs[pos] = c
    _, w64 = gr.f64_copy(wf)
    p = np.exp(2 * gr.log_amp_f64(w64, _states(hil, all_keys)))
    expect = p / p.sum() * obs.sum()
    m = expect >= 5
    chi2 = ((obs[m] - expect[m]) ** 2 / expect[m]).sum() + (obs[~m].sum() - expect[~m].sum()) ** 2 / max(expect[~m].sum(), 1e-9)
    assert stats.chi2.sf(chi2, m.sum()) > 1e-4, (chi2, m.sum())


# ------------------------------------------------------------------------------------------------------------ gradients
def _grads(wf):
    return {n: p.grad.detach().double().cpu().numpy().copy() for n, p in wf.model.named_parameters()}


def _zero_grad(wf):
    for p in wf.model.parameters():
        p.grad = None


def _both_forms(fused, wf, kd, e_d, w_d, s_d):
    _zero_grad(wf)
    fused._grad_flat = None
    _, saved = fused.forward_saved(kd)
    fused.backward_from_local_energy(saved, e_d, w_d, s_d)
    g1 = _grads(wf)
    _zero_grad(wf)
    fused._grad_flat = None
    _, saved = fused.forward_saved(kd)
    g, _ = fused.vmc_loss_grad(e_d, w_d, s_d, with_energy=True)
    fused.backward_saved(saved, g)
    g2 = _grads(wf)
    torch.cuda.synchronize()
    return g1, g2


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("name,sym,ha", [("LiF", True, 64), ("LiF", False, 64), ("Li2O", True, 128), ("syn32_8_8", False, 32),
                                         ("H2O_6-31G", True, 16)])
def test_training_step_gradients_against_float64(name, sym, ha, capsys):
    _threads()
    hil, wf = _net(name, sym=sym, ha=ha, seed=11)
    fused = wf.fused()
    assert fused is not None and fused.comb
    cuts = [m for m in (1, 64, 1000, 10000) if m <= hil.size]
    keys = gr.random_keys(hil, max(cuts), seed=9)
    _, w64 = gr.f64_copy(wf)
    rs = np.random.RandomState(1)
    worst = 0.0
    for M in cuts:
        k = np.sort(keys[:M])
        st = _states(hil, k)
        lp64, margin = gr.log_psi_and_kink_margin(w64, st)
        w = rs.random_sample(M) + 0.1
        w[margin < TAU] = 0.0
        w /= max(w.sum(), 1e-300)
        e = rs.normal(-7.0, 1.0, M) + 1j * rs.normal(0.0, 0.3, M)
        sums = np.array([(w * e.real).sum(), (w * e.imag).sum(), (w * e.real ** 2).sum(), w.sum()])
        g_dev = gr.loss_grad_f32_emulated(e, w, sums).astype(np.float64)
        want = gr.grad_f64(w64, st, g_dev, lp=lp64)
        g1, g2 = _both_forms(fused, wf, _kdev(k), _dev(np.stack([e.real, e.imag], -1)), _dev(w), _dev(sums))
        for pname in want:
            assert np.array_equal(g1[pname], g2[pname]), (M, pname)
            scale = np.abs(want[pname]).max()
            err = np.abs(g1[pname] - want[pname]).max() / scale if scale > 0 else np.abs(g1[pname]).max()
            assert err <= GRAD_BOUND, (name, sym, ha, M, pname, err)
            worst = max(worst, err)
    with capsys.disabled():
        print(f"\n[comb] gradients {name} sym={sym} Ha={ha}: worst {worst:.2e} of the tensor scale over M = {cuts}")


@pytest.mark.parametrize("mol,fix", FIXTURES)
def test_training_step_gradients_against_the_reference(mol, fix):
    z, hil, wf = _fixture(mol, fix)
    fused = wf.fused()
    k = z["samp_keys"].astype(np.uint64)
    order = np.argsort(k)
    w = z["samp_counts"].astype(np.float64)[order]
    w /= w.sum()
    e = z["sgd_eloc_c128"][order]
    sums = np.array([(w * e.real).sum(), (w * e.imag).sum(), (w * e.real ** 2).sum(), w.sum()])
    g1, g2 = _both_forms(fused, wf, _kdev(k[order]), _dev(np.stack([e.real, e.imag], -1)), _dev(w), _dev(sums))
    for name in g1:
        assert np.array_equal(g1[name], g2[name]), name
        g_ref = z["grad:" + name]
        scale = max(1e-3, np.abs(g_ref).max())
        assert np.max(np.abs(g1[name] - g_ref)) < 2e-3 * scale, (name, np.max(np.abs(g1[name] - g_ref)) / scale)


def test_amp_backward_differentiates_log_abs_psi_only():
    """naqs_net_amp_backward on a combined handle: the gradient of sum_i g_i log|psi_i| in the flat layout — the phase rows of
    the last block get zero, everything else the float64 gradient of log|psi| alone."""
    _threads()
    hil, wf = _net("LiF", sym=True, seed=2)
    fused = wf.fused()
    keys = np.sort(gr.random_keys(hil, 3000, seed=4))
    st = _states(hil, keys)
    _, w64 = gr.f64_copy(wf)
    lp64, margin = gr.log_psi_and_kink_margin(w64, st)
    g = np.random.RandomState(3).normal(size=len(keys))
    g[margin < TAU] = 0.0
    want = gr.grad_f64(w64, st, np.stack([g, np.zeros_like(g)], -1), lp=lp64)
    flat = torch.empty(fused.n_amp_params, dtype=torch.float32, device="cuda")
    gd = torch.as_tensor(g, dtype=torch.float32, device="cuda")
    kd = _kdev(keys)
    from naqs_amd.hamiltonian import _stream_ptr
    assert fused._lib.naqs_net_amp_backward(fused._h, len(keys), kd.data_ptr(), gd.data_ptr(), flat.data_ptr(),
                                            _stream_ptr(fused.device)) == 0
    got = flat.double().cpu().numpy()
    off = 0
    for name, p in wf.model.named_parameters():
        n = p.numel()
        gp = got[off:off + n].reshape(p.shape)
        off += n
        scale = np.abs(want[name]).max()
        assert np.abs(gp - want[name]).max() <= GRAD_BOUND * max(scale, 1e-30), name
    last = wf.model.amp_layers[-1].linears()[1]
    assert not torch.equal(last.weight, torch.zeros_like(last.weight))
    assert np.all(got[off - 3 - 3 * 64 - 5: off - 3 - 5] == 0) and np.all(got[off - 3:] == 0)     # W2 phase rows, b2 phase


# ----------------------------------------------------------------------------------------------------------------- loop
def _opt(mol, wf, tmp, **kw):
    from naqs_amd import packing
    from naqs_amd.optimizer import PartialSamplingOptimizer
    from test_nade import ELECTRONS
    from test_optimizer import ADAM
    N, na, nb = ELECTRONS[mol]
    ham = packing.load_packed(os.path.join(ROOT, "tests", "golden", f"ham_{mol}.npz"))
    args = dict(n_samples=100000, n_samples_max=1e12, n_unq_samples_min=10, n_unq_samples_max=1e5, log_exact_energy=False,
                wavefunction=wf, qubit_hamiltonian=ham, pre_compute_H=False, n_electrons=na + nb, n_alpha_electrons=na,
                n_beta_electrons=nb, normalise_psi=True, grad_clip_factor=None, optimizer=torch.optim.Adam,
                optimizer_args=[dict(a) for a in ADAM], save_loc=str(tmp), pauli_hamiltonian_dtype=np.float64, seed=5)
    args.update(kw)
    return PartialSamplingOptimizer(**args)


@pytest.mark.parametrize("mol,sym", [("N2", True), ("H2O", False)])
def test_vmc_run_equals_step_by_step(mol, sym, tmp_path, monkeypatch, capsys):
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.optimizer import LogKey
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    from test_nade import ELECTRONS
    N, na, nb = ELECTRONS[mol]
    runs = {}
    for run, onecall in (("1", "1"), ("0", "1"), ("0", "0")):
        monkeypatch.setenv("NAQS_TRAIN_RUN", run)
        monkeypatch.setenv("NAQS_TRAIN_ONECALL", onecall)
        hil = Hilbert.get(N, na, nb, encoding=Encoding.SIGNED, make_basis=True)
        torch.manual_seed(3)
        wf = NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, amp_hidden_size=[64], phase_hidden_size=[64],
                                       use_amp_spin_sym=sym, use_phase_spin_sym=sym, aggregate_phase=False,
                                       combined_amp_phase_blocks=True, n_alpha_electrons=na, n_beta_electrons=nb)
        opt = _opt(mol, wf, tmp_path / (run + onecall))
        assert wf.fused() is not None and wf.fused().comb
        assert opt._can_onecall() == (onecall == "1") and opt._can_run_in_library() == (run == "1")
        opt.run(n_epochs=20, save_freq=None, save_final=False, output_freq=10)
        assert "not available" not in capsys.readouterr().out
        runs[run + onecall] = dict(e=np.array(opt.log[LogKey.E_LOC]), n=np.array(opt.log[LogKey.N_UNIQUE_SAMP]),
                                   p=wf.flatten_parameters().clone(), t=opt.optimizer._t)
    a = runs["11"]
    assert a["t"] == 20 and np.isfinite(a["e"]).all()
    for k in ("01", "00"):
        b = runs[k]
        assert np.array_equal(a["e"], b["e"]) and np.array_equal(a["n"], b["n"]) and torch.equal(a["p"], b["p"]), k


def test_shard_calls_refuse_combined_handles():
    from naqs_amd.hamiltonian import _stream_ptr
    hil, wf = _net("LiF", seed=1)
    fused = wf.fused()
    lib = fused._lib
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    info = (ctypes.c_int64 * 3)(0, 0, 0)
    assert lib.naqs_vmc_shard_sample_forward(fused._h, 1000, 1, 1000, 0, 1000, 0, 2, p, p, p, p, p, info,
                                             _stream_ptr(fused.device)) == -4
    assert lib.naqs_vmc_shard_update(fused._h, p, p, p, p, 1e-3, 0.9, 0.99, 1e-15, 0.0, 1, _stream_ptr(fused.device)) == -4


def test_h2o_training_to_convergence(tmp_path, capsys):
    """test_config3_gpu.py's run (the batch script's flags, the default learning-rate schedule, 10 000 steps, seed 111) with
    -comb_amp_phase, on the HIP kernels (no fallback notice): the sampled-subspace diagonalisation within 0.1 mHa of FCI and never
    below it, the final <E_loc> above FCI - 1e-5 Ha and within 1 mHa of it."""
    import json
    import sys
    from conftest import GOLDEN, PKG
    from test_config3_gpu import FLAGS
    sys.path.insert(0, PKG)
    from experiments import _base
    kat = json.load(open(os.path.join(GOLDEN, "kat.json")))
    res = _base.run(molecule=None, out=None, number=1, lr=-1, n_samps=1e7, n_samps_max=1e12, n_unq_samps_min=1e4,
                    n_unq_samps_max=1e5, n_hid=128, n_layer=1, reweight_samples_by_psi=False, n_train=10000, n_pretrain=0,
                    output_freq=25, save_freq=-1, load_hamiltonian=False, overwrite_hamiltonian=False,
                    presolve_hamiltonian=False, cont=False, n_excitations_max=-1, use_amp_spin_sym=True,
                    use_phase_spin_sym=False, comb_amp_phase=False, aggregate_phase=True, restrict_H=True, reset_opt=False,
                    argv=["-m", os.path.join(GOLDEN, "ham_H2O.npz"), "-o", str(tmp_path / "run"), "-s", "111"] + FLAGS
                    + ["-comb_amp_phase"])
    out = capsys.readouterr().out
    r = res[0]
    fci = kat["fci"]["H2O"]
    with capsys.disabled():
        print(f"\n[comb] H2O -comb_amp_phase: final <E_loc> {r['final']:.8f} Ha, subspace {r['eig']:.8f} Ha ({r['n_unq']} states), "
              f"FCI {fci:.8f} Ha, {r['time']:.1f} s for 10 000 steps")
    assert "fused HIP network kernels not available" not in out
    assert -1e-8 < r["eig"] - fci < 1e-4, (r["eig"], fci)
    assert -1e-5 < r["final"] - fci < 1e-3, (r["final"], fci)
