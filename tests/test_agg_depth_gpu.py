"""Aggregate-phase networks with 2..4 hidden layers in every block (naqs_net_create_agg_layers) on the MI355X: run.py's default
ansatz with -n_layer L, which the per-pair phase blocks follow (-n_layer_phase / -n_hid_phase default to -n_layer / -n_hid).

* log psi against the float64 copy of the network (tests/grad_reference.py) at L = 2, 3, 4, widths 16..128 (one case with
  Ha != Hp), with and without -phase_sym and amplitude symmetry, PARTIAL / FULL / NONE masking, P = 2, 6, 10, 16, at 1, 15, 16,
  17, 1000 and 10^4 rows.  Bounds, per row:
    log|psi|: P L A + B |log|psi|_f64|, A = 4e-7, B = 1e-7 — test_amp_depth_gpu.py's deep bound (the amplitude set is the
              same kernel code on the same numbers).
    phase:    P L A + B |phase_f64|, the same form and constants.  Each pair's phase is a raw output of an L-layer block on the
              f32 matrix cores: no conditional, so per block the same float32 roundings of the layers' sums as an amplitude
              block's outputs (which the log-softmax passes on unamplified), allowed A per layer; the float32 sum of the P
              phases adds B |phase|.  The sign shift is float32 pi on both sides (nade.py's tensor), exact in the copy.
  The worst ratio to each bound is printed.  naqs_logpsi_eloc must give the same log psi and the E_loc of ham.local_energy, the
  training forward the same bits; the merged launch (agg_deep_kernel, Ha == Hp) and the two launches (NAQS_AGG_MERGE=6) the
  same bits.
* the sampler: draws (keys, counts, probs) bit for bit those of a naqs_net_create_amp_layers handle with the same amplitude
  parameters; chi^2 against exact |psi|^2 on LiH and H2O at L = 2.
* both training-step call forms against float64 gradients of the loss gradient the device forms (2e-5 of each tensor's scale —
  at least a tenth of its gradient under |g|, where the seeds cancel; rows within 1e-5 of a ReLU kink get w = 0), bit for bit equal to each other and to the unmerged backward (NAQS_AGG_MERGE=5),
  at the row counts where the backward changes path.
* naqs_vmc_run over 20 steps equal to the step-by-step library calls.
* the reference's fixtures (tests/golden/aggdepth_*.npz, make_golden_agg_depth.py): log psi within 5e-5, gradients within 2e-3
  of grad:*, the parameters after one _SGD_step.
* H2O trained with run.py's defaults plus -n_layer 2 (10 000 steps, seed 111), on the kernels, to 1 mHa of FCI.
* what stays on the PyTorch modules: mixed depths, combined blocks, odd widths — with the messages the older tests pin.
"""
import os

import numpy as np
import pytest

import grad_reference as gr
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A, B = 4e-7, 1e-7
TAU, GRAD_BOUND = 1e-5, 2e-5
ROWS = [1, 15, 16, 17, 1000, 10000]


def _threads():
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))


def _net(name, L, ha, hp=None, sym=True, phase_sym=False, masking="PARTIAL", seed=0, device="cuda"):
    """(hilbert, network) on sector `name` of grad_reference.SECTORS: the aggregate phase, L hidden layers of `ha` units in every
    amplitude block and of `hp` (default `ha`) in every phase block, default-initialised from `seed`."""
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.nade import NadeMasking
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    _, N, na, nb, _ = gr.sector(name)
    hil = Hilbert.get(N, na, nb, encoding=Encoding.SIGNED)
    torch.manual_seed(seed)
    wf = NAQSComplex_NADE_orbitals(hil, device=device, qubit_ordering=-1, masking=NadeMasking[masking],
                                   amp_hidden_size=[ha] * L, phase_hidden_size=[hp or ha] * L, use_amp_spin_sym=sym,
                                   use_phase_spin_sym=phase_sym, aggregate_phase=True, n_alpha_electrons=na, n_beta_electrons=nb)
    return hil, wf


def _kdev(keys):
    return torch.as_tensor(np.asarray(keys).astype(np.int64), device="cuda")


def _states(hil, keys):
    return hil.idx2state(torch.as_tensor(np.asarray(keys).astype(np.int64)))


def _form(L, ha, hp, merged=True):
    if merged and ha == hp:
        return f"agg_deep_kernel<{ha // 16}, L={L}> + agg_finish_kernel"
    return f"amp_deep_kernel<{ha // 16}, L={L}> + amp_deep_raw_kernel<{hp // 16}, L={L}> + agg_finish_kernel"


def _last_forward(fused):
    return fused.last_kernel().split(";")[0]


def _ratios(got, want, P, L):
    got = np.asarray(got, np.float64)
    assert not np.isnan(got).any()
    ninf = ~np.isfinite(want[:, 0])
    assert np.array_equal(ninf, got[:, 0] == -np.inf)
    ok = ~ninf
    r0 = (np.abs(got[ok, 0] - want[ok, 0]) / (P * L * A + B * np.abs(want[ok, 0]))).max(initial=0.0)
    r1 = (np.abs(got[ok, 1] - want[ok, 1]) / (P * L * A + B * np.abs(want[ok, 1]))).max(initial=0.0)
    return r0, r1


def _ham_for(name, keys):
    from naqs_amd import hamiltonian
    from test_pairs_gpu import _row_ham
    return hamiltonian.DevicePauliHamiltonian(_row_ham(name, np.asarray(keys, np.uint64)), device="cuda")


# name -> (sector, L, Ha, Hp, options)
FORWARD = {
    "H2_L2_32": ("H2", 2, 32, 32, {}),
    "LiH_L3_64_phasesym": ("LiH", 3, 64, 64, {"phase_sym": True}),
    "LiH_L4_32_full_noampsym": ("LiH", 4, 32, 32, {"masking": "FULL", "sym": False}),
    "LiF_L2_128": ("LiF", 2, 128, 128, {}),
    "LiF_L2_64_32_nomask": ("LiF", 2, 64, 32, {"masking": "NONE"}),
    "LiF_L3_32_phasesym_noampsym": ("LiF", 3, 32, 32, {"phase_sym": True, "sym": False}),
    "syn32_L2_64": ("syn32_8_8", 2, 64, 64, {}),
    "syn32_L4_128_phasesym_full": ("syn32_8_8", 4, 128, 128, {"phase_sym": True, "masking": "FULL"}),
}


@pytest.mark.parametrize("case", list(FORWARD))
def test_forward_against_float64(case, monkeypatch, capsys):
    _threads()
    name, L, ha, hp, opt = FORWARD[case]
    hil, wf = _net(name, L, ha, hp, **opt)
    fused = wf.fused()
    assert fused is not None and fused.aggregate and fused.amp_depth == L
    assert "not available" not in capsys.readouterr().out
    assert fused.n_params == sum(p.numel() for p in wf.model.parameters())
    assert fused.n_amp_params == sum(p.numel() for blk in wf.model.amp_layers for p in blk.parameters())
    rows = sorted({min(m, hil.size) for m in ROWS})
    keys = gr.random_keys(hil, max(rows), seed=5)
    _, w64 = gr.f64_copy(wf)
    want = gr.log_psi_f64(w64, _states(hil, keys))
    P = hil.N // 2
    worst = [0.0, 0.0]
    for M in rows:
        kd = _kdev(keys[:M])
        monkeypatch.delenv("NAQS_AGG_MERGE", raising=False)
        got = fused.log_psi(kd)
        torch.cuda.synchronize()
        assert _last_forward(fused) == _form(L, ha, hp), (M, fused.last_kernel())
        r0, r1 = _ratios(got.cpu().numpy(), want[:M], P, L)
        assert r0 <= 1 and r1 <= 1, (case, M, r0, r1)
        worst = [max(worst[0], r0), max(worst[1], r1)]
        lp2, _ = fused.forward_saved(kd)                      # the training forward: the same launches, the same bits
        torch.cuda.synchronize()
        assert torch.equal(lp2, got)
        monkeypatch.setenv("NAQS_AGG_MERGE", "6")             # the two-launch form
        got2 = fused.log_psi(kd)
        torch.cuda.synchronize()
        assert _last_forward(fused) == _form(L, ha, hp, merged=False), (M, fused.last_kernel())
        assert torch.equal(got2, got), M
    monkeypatch.delenv("NAQS_AGG_MERGE", raising=False)
    with capsys.disabled():
        print(f"\n[agg depth] {case}: worst error {worst[0]:.2f} (log|psi|) and {worst[1]:.2f} (phase) x bound over M = {rows}")
    # naqs_logpsi_eloc: the same log psi, the E_loc of ham.local_energy
    M = max(rows)
    k = np.sort(keys[:M])
    kd = _kdev(k)
    ham = _ham_for(name, k)
    lp = fused.log_psi(kd)
    lp_e, e = fused.log_psi_and_local_energy(ham, kd)
    torch.cuda.synchronize()
    assert torch.equal(lp, lp_e)
    e_ref = ham.local_energy(kd, lp, kind="log_psi")
    assert torch.equal(e.reshape(e_ref.shape), e_ref)


def test_default_n2_command_with_two_layers_is_fused(capsys):
    """run.py's N2 network (-n_hid 128, P = 10) with -n_layer 2 gets a fused handle (it fell back to PyTorch modules before)."""
    hil, wf = _net("LiF", 2, 128)
    fused = wf.fused()
    assert fused is not None and fused.aggregate and fused.amp_depth == 2
    assert "not available" not in capsys.readouterr().out


# -------------------------------------------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("name,L,ha,hp,phase_sym", [("LiH", 2, 64, 32, False), ("LiF", 3, 128, 128, True), ("syn32_8_8", 2, 32, 32, False)])
def test_sampler_draws_what_the_amplitude_handle_draws(name, L, ha, hp, phase_sym):
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    hil, wf = _net(name, L, ha, hp, phase_sym=phase_sym, seed=3)
    _, N, na, nb, _ = gr.sector(name)
    torch.manual_seed(9)
    single = NAQSComplex_NADE_orbitals(Hilbert.get(N, na, nb, encoding=Encoding.SIGNED), device="cuda", qubit_ordering=-1,
                                       amp_hidden_size=[ha] * L, phase_hidden_size=[64, 64], use_amp_spin_sym=True,
                                       aggregate_phase=False, n_alpha_electrons=na, n_beta_electrons=nb)
    single.model.amp_layers.load_state_dict(wf.model.amp_layers.state_dict())
    fa, fs = wf.fused(), single.fused()
    assert fa is not None and fs is not None and fa.aggregate and not fs.aggregate and fs.amp_depth == L
    for seed in (11, 12):
        a = fa.sample(10 ** 5, seed=seed, max_unique=400000)
        b = fs.sample(10 ** 5, seed=seed, max_unique=400000)
        torch.cuda.synchronize()
        assert "sample_expand_deep_kernel" in fa.last_kernel()
        assert len(a[0]) > 0 and all(torch.equal(x, y) for x, y in zip(a, b)), seed


@pytest.mark.parametrize("mol,n", [("LiH", 2_000_000), ("H2O", 5_000_000)])
def test_sampler_distribution(mol, n):
    from scipy import stats
    import test_amp_depth_gpu as tad
    hil, wf = tad._net(mol, 2, 64, aggregate=True, phase_hidden=(64, 64), seed=7)
    fused = wf.fused()
    assert fused is not None and fused.aggregate and fused.amp_depth == 2
    keys, counts, probs = fused.sample(n, seed=20240607, max_unique=100000)
    k, c = keys.cpu().numpy(), counts.cpu().numpy()
    assert np.all(np.diff(k) > 0) and hil.is_physical(k).all() and (c > 0).all()
    all_keys = np.sort(hil._all_keys())
    lp = fused.log_psi(torch.as_tensor(all_keys, device="cuda"))[:, 0].double().cpu().numpy()
    p = np.exp(2.0 * lp)
    p_phys, total = p.sum(), c.sum()
    assert total <= n and abs(total - n * p_phys) < 6 * np.sqrt(n * p_phys * (1 - p_phys)) + 1
    pos = np.searchsorted(all_keys, k)
    assert np.array_equal(all_keys[pos], k)
    rel = np.abs(probs.cpu().numpy().astype(np.float64) / p[pos] - 1)
    assert (rel <= tad._probs_bound(lp[pos], hil.N // 2)).all(), rel.max()
    obs = np.zeros(len(all_keys))
    obs[pos] = c
    expect = p / p_phys * total
    m = expect >= 5
    chi2 = ((obs[m] - expect[m]) ** 2 / expect[m]).sum() + (obs[~m].sum() - expect[~m].sum()) ** 2 / max(expect[~m].sum(), 1e-9)
    assert stats.chi2.sf(chi2, m.sum()) > 1e-4, (chi2, m.sum())


# ------------------------------------------------------------------------------------------------------------ gradients
def _grads(wf):
    return {n: p.grad.detach().double().cpu().numpy().copy() for n, p in wf.model.named_parameters()}


def _zero_grad(wf):
    for p in wf.model.parameters():
        p.grad = None


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


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


GRAD = {
    "H2_L2_16": ("H2", 2, 16, 16, {}),
    "LiF_L2_64": ("LiF", 2, 64, 64, {}),
    "LiF_L3_32_64_phasesym": ("LiF", 3, 32, 64, {"phase_sym": True}),
    "syn32_L4_128_noampsym": ("syn32_8_8", 4, 128, 128, {"sym": False}),
    "syn32_L2_32_phasesym_full": ("syn32_8_8", 2, 32, 32, {"phase_sym": True, "masking": "FULL"}),
}


@pytest.mark.parametrize("case", list(GRAD))
def test_training_step_gradients_against_float64(case, monkeypatch, capsys):
    import test_amp_depth_gpu as tad
    _threads()
    name, L, ha, hp, opt = GRAD[case]
    hil, wf = _net(name, L, ha, hp, seed=11, **opt)
    fused = wf.fused()
    assert fused is not None and fused.train_mode == "hip"
    cuts = sorted({min(m, hil.size) for m in tad._grad_cuts()})
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
        # the seeds sum to zero over the rows, so a parameter with the same derivative on every row (pair 0's block, whose input
        # is constant, on rows that share its outcome — H2 at M = 2) has a float64 gradient that is rounding residue: such a
        # tensor is measured against a tenth of its gradient under |g| (the size of the terms its float32 sums add)
        want_abs = gr.grad_f64(w64, st, np.abs(g_dev))
        args = (fused, wf, _kdev(k), _dev(np.stack([e.real, e.imag], -1)), _dev(w), _dev(sums))
        monkeypatch.delenv("NAQS_AGG_MERGE", raising=False)
        g1, g2 = _both_forms(*args)
        last = fused.last_kernel()
        assert ("agg_deep_backward_kernel" in last) == (ha == hp) and ("amp_deep_backward_raw_kernel" in last) == (ha != hp), last
        monkeypatch.setenv("NAQS_AGG_MERGE", "5")             # the unmerged backward: two launches on split columns
        g3, _ = _both_forms(*args)
        assert "amp_deep_backward_raw_kernel" in fused.last_kernel()
        for pname in want:
            assert np.array_equal(g1[pname], g2[pname]) and np.array_equal(g1[pname], g3[pname]), (M, pname)
            scale = max(np.abs(want[pname]).max(), 0.1 * np.abs(want_abs[pname]).max())
            err = np.abs(g1[pname] - want[pname]).max() / scale if scale > 0 else np.abs(g1[pname]).max()
            assert err <= GRAD_BOUND, (case, M, pname, err)
            worst = max(worst, err)
    monkeypatch.delenv("NAQS_AGG_MERGE", raising=False)
    with capsys.disabled():
        print(f"\n[agg depth] gradients {case}: worst {worst:.2e} of the tensor scale over M = {cuts}")


def test_gradients_are_deterministic():
    hil, wf = _net("LiF", 2, 64, seed=4)
    fused = wf.fused()
    k = np.sort(gr.random_keys(hil, 5000, seed=2))
    rs = np.random.RandomState(0)
    w = rs.random_sample(len(k))
    w /= w.sum()
    e = rs.normal(-7.0, 1.0, len(k)) + 1j * rs.normal(0.0, 0.3, len(k))
    sums = np.array([(w * e.real).sum(), (w * e.imag).sum(), (w * e.real ** 2).sum(), w.sum()])
    args = (fused, wf, _kdev(k), _dev(np.stack([e.real, e.imag], -1)), _dev(w), _dev(sums))
    a, _ = _both_forms(*args)
    b, _ = _both_forms(*args)
    assert all(np.array_equal(a[n], b[n]) for n in a)


# ----------------------------------------------------------------------------------------------------------------- loop
@pytest.mark.parametrize("mol,L,phase_sym", [("N2", 2, False), ("H2O", 3, True)])
def test_vmc_run_equals_step_by_step(mol, L, phase_sym, tmp_path, monkeypatch, capsys):
    """naqs_vmc_run over 20 steps against one naqs_vmc_step per step and against the step-by-step library calls: energies,
    sample counts and parameters bit for bit."""
    import test_amp_depth_gpu as tad
    from naqs_amd.optimizer import LogKey
    runs = {}
    for run, onecall in (("1", "1"), ("0", "1"), ("0", "0")):
        monkeypatch.setenv("NAQS_TRAIN_RUN", run)
        monkeypatch.setenv("NAQS_TRAIN_ONECALL", onecall)
        hil, wf = tad._net(mol, L, 64, aggregate=True, phase_hidden=(32,) * L, phase_sym=phase_sym, seed=3)
        opt = tad._opt(mol, wf, tmp_path / (run + onecall))
        assert wf.fused() is not None and wf.fused().aggregate
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


def test_shard_calls_refuse():
    import ctypes
    hil, wf = _net("LiH", 2, 32)
    fused = wf.fused()
    info = (ctypes.c_int64 * 3)()
    nul = ctypes.c_void_p(None)
    buf = torch.zeros(fused.n_params, dtype=torch.float32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    st = fused._lib.naqs_vmc_shard_sample_forward(fused._h, 1000, 1, 100, 0, 100, 0, 2, nul, nul, nul, nul, p, info, nul)
    assert st == -4                                          # NAQS_ERR_UNSUPPORTED, before anything is launched
    assert fused._lib.naqs_vmc_shard_update(fused._h, p, p, p, p, 1e-3, 0.9, 0.99, 1e-15, 0.0, 1, nul) == -4


# ------------------------------------------------------------------------------------------------------------- fixtures
FIXTURES = [("LiH", "LiH"), ("LiH", "LiH_phasesym"), ("N2", "N2")]


def _fixture(mol, fix):
    """The network a tests/golden/aggdepth_*.npz fixture was recorded with, its parameters loaded (make_golden_agg_depth.py)."""
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.nade import NadeMasking
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    from test_nade import ELECTRONS
    z = golden(f"aggdepth_{fix}.npz")
    N, na, nb = ELECTRONS[mol]
    hil = Hilbert.get(N, na, nb, encoding=Encoding.SIGNED, make_basis=True)
    L = int(z["cfg_n_layer_phase"])
    wf = NAQSComplex_NADE_orbitals(hil, qubit_ordering=-1, masking=NadeMasking(int(z["cfg_masking"])),
                                   amp_hidden_size=[int(z["cfg_n_hid"])] * L, phase_hidden_size=[int(z["cfg_n_hid_phase"])] * L,
                                   use_amp_spin_sym=bool(z["cfg_use_amp_spin_sym"]), use_phase_spin_sym=bool(z["cfg_use_phase_spin_sym"]),
                                   aggregate_phase=True, n_alpha_electrons=na, n_beta_electrons=nb, device="cuda")
    sd = {k[3:]: torch.tensor(z[k]) for k in z.files if k.startswith("sd:")}
    assert set(sd) == set(wf.model.state_dict()), "state_dict keys must match the reference's"
    wf.model.load_state_dict(sd)
    return z, hil, wf


@pytest.mark.parametrize("mol,fix", FIXTURES)
def test_fixture_log_psi_matches_the_reference(mol, fix, capsys):
    z, hil, wf = _fixture(mol, fix)
    fused = wf.fused()
    assert fused is not None and fused.aggregate and fused.amp_depth == 2
    assert "not available" not in capsys.readouterr().out
    lp = fused.log_psi(_kdev(z["eval_keys"]))
    torch.cuda.synchronize()
    assert np.max(np.abs(lp.cpu().numpy() - z["eval_log_psi"])) < 5e-5


@pytest.mark.parametrize("mol,fix", FIXTURES)
def test_fixture_gradients_match_the_reference(mol, fix):
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


@pytest.mark.parametrize("mol,fix", FIXTURES)
def test_fixture_sgd_step_matches_the_reference(mol, fix, tmp_path):
    """One _SGD_step against the reference's, as test_variants_gpu.py checks it: E, Var and the parameters after one Adam step
    (lr sign(g) with eps = 1e-15: entries whose reference gradient is rounding noise may flip)."""
    from test_variants_gpu import _opt
    from naqs_amd.flat_adam import FlatAdam
    z, hil, wf = _fixture(mol, fix)
    opt = _opt(mol, wf, tmp_path)
    assert wf.fused() is not None and isinstance(opt.optimizer, FlatAdam)
    states = torch.tensor(z["samp_states"], device="cuda")
    counts = torch.tensor(z["samp_counts"], device="cuda")
    keys = hil.state2idx(states).squeeze(-1)
    E, var = opt._SGD_step(states, keys, None, sample_weights=counts.double() / counts.sum().double())
    assert abs(E - float(z["sgd_E"])) < 2e-5 * max(1, abs(E))
    assert abs(var - float(z["sgd_Var"])) < 1e-3 * max(1, abs(var))
    for name, p in wf.model.named_parameters():
        d = np.abs(p.detach().cpu().numpy() - z["sd_after:" + name])
        flipped = d >= 2e-5
        if flipped.any():
            g = np.abs(z["grad:" + name])
            assert flipped.sum() <= max(2, 1e-4 * d.size), (name, int(flipped.sum()))
            assert d[flipped].max() < 2.1e-3 and g[flipped].max() <= 1e-3 * g.max(), (name, d[flipped].max())


# ----------------------------------------------------------------------------------------------------------- end to end
def test_h2o_default_command_with_two_layers_trains_to_fci(tmp_path, capsys):
    """run.py's defaults (the aggregate phase, -n_hid 128, 10 000 steps) plus -n_layer 2 on H2O, seed 111: on the kernels (no
    fallback notice), the final <E_loc> and the sampled-subspace energy within 1 mHa of FCI (test_config3_gpu.py's criterion)."""
    import json
    import sys
    from conftest import GOLDEN, PKG
    sys.path.insert(0, PKG)
    from experiments import _base
    kat = json.load(open(os.path.join(GOLDEN, "kat.json")))
    res = _base.run(molecule=None, out=None, number=1, lr=-1, n_samps=1e7, n_samps_max=1e12, n_unq_samps_min=1e4,
                    n_unq_samps_max=1e5, n_hid=128, n_layer=1, reweight_samples_by_psi=False, n_train=10000, n_pretrain=0,
                    output_freq=25, save_freq=-1, load_hamiltonian=False, overwrite_hamiltonian=False,
                    presolve_hamiltonian=False, cont=False, n_excitations_max=-1, use_amp_spin_sym=True,
                    use_phase_spin_sym=False, comb_amp_phase=False, aggregate_phase=True, restrict_H=True, reset_opt=False,
                    argv=["-m", os.path.join(GOLDEN, "ham_H2O.npz"), "-o", str(tmp_path / "run"), "-s", "111", "-n_layer", "2"])
    out = capsys.readouterr().out
    r = res[0]
    fci = kat["fci"]["H2O"]
    with capsys.disabled():
        print(f"\n[agg depth] H2O default command -n_layer 2: final <E_loc> {r['final']:.8f} Ha, subspace {r['eig']:.8f} Ha "
              f"({r['n_unq']} states), FCI {fci:.8f} Ha, {r['time']:.1f} s for 10 000 steps")
    assert "fused HIP network kernels not available" not in out
    assert -1e-5 < r["final"] - fci < 1e-3, (r["final"], fci)
    assert -1e-8 < r["eig"] - fci < 1e-3, (r["eig"], fci)


# ----------------------------------------------------------------------------------------------------------- boundaries
def _boundary(amp, phase, comb=False):
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    hil = Hilbert.get(12, 2, 2, encoding=Encoding.SIGNED)
    return NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, amp_hidden_size=list(amp), phase_hidden_size=list(phase),
                                     aggregate_phase=True, combined_amp_phase_blocks=comb, n_alpha_electrons=2, n_beta_electrons=2)


@pytest.mark.parametrize("amp,phase,comb,text", [
    ((32, 32), (32,), False, "amplitude blocks need exactly one hidden layer"),          # mixed depths
    ((32, 32), (32, 32, 32), False, "amplitude blocks need exactly one hidden layer"),
    ((32,), (32, 32), False, "aggregate_phase"),
    ((32, 32), (32, 64), False, "aggregate_phase"),                                      # unequal phase widths
    ((40, 40), (32, 32), False, "amplitude hidden width 40"),                           # odd widths
    ((32, 32), (40, 40), False, "aggregate_phase"),
    ((144, 144), (144, 144), False, "amplitude hidden width 144"),
    ((32, 32), (32, 32), True, "combined amplitude-phase blocks"),                      # combined blocks
    ((32,), (32,), True, "combined amplitude-phase blocks"),
])
def test_outside_the_family_stays_on_torch(amp, phase, comb, text, capsys):
    wf = _boundary(amp, phase, comb)
    assert wf.fused() is None
    out = capsys.readouterr().out
    assert "fused HIP network kernels not available" in out and text in out, out
