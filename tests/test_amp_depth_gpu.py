"""Amplitude blocks with 2..4 hidden layers (naqs_net_create_amp_layers; naqs_amp_deep.hpp) on the MI355X.

* log psi against the float64 copy of the network (tests/grad_reference.py) for depths 2, 3, 4, widths 32, 64, 128, the LiH,
  H2O and N2 spaces and a 30-qubit net, with and without amplitude spin symmetry, under every masking mode and with -phase_sym,
  at the row counts where select_form changes kernel (test_forward_f64_gpu.py derives them from the source and the CU count).
  Bound: |d log|psi|| <= P L A + B |log|psi|_f64| with A = 4e-7, B = 1e-7 (P pairs, L hidden layers).  The deep blocks run on
  the f32 matrix cores with no split format, so each layer adds float32 rounding of its sums only; A is the per-pair allowance
  of the depth-1 forward (test_forward_f64_gpu.py: LOG_PAIR) taken once per layer, B the float32 sum of the P conditionals.
  The phase is the depth-1 kernels' (PHASE_REL of the table's largest |phase|).  Every case asserts the launches'
  names; naqs_logpsi_eloc must give the same log psi and the E_loc of ham.local_energy.
* the sampler: chi^2 against exact |psi|^2 (LiH, H2O; depths 2 and 3), same seed -> same draw, probs = exp(2 log|psi|) of the
  log-psi call to 1e-6 + 2 P 2^-24 |log|psi|| relative (the float32 sum inside log|psi|; 1e-6 alone was missed by 1.2e-6 on LiH);
* both training-step call forms against float64 gradients of the loss gradient the device forms (2e-5 of each tensor's scale;
  rows within 1e-5 of a ReLU kink get w = 0), bit for bit equal to each other, at the row counts where the backward changes
  path; the error of float32 autograd on the CPU is printed beside;
* naqs_vmc_run over 20 steps equal to the step-by-step library calls;
* what stays outside: depth 5, mixed widths, aggregate phase with deep blocks.
"""
import os

import numpy as np
import pytest

import grad_reference as gr
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LOG_LAYER_PAIR, LOG_REL = 4e-7, 1e-7
PHASE_REL, PHASE_FLOOR = 5e-6, 1e-3
TAU, GRAD_BOUND = 1e-5, 2e-5


def _net(mol, depth, ha, sym=True, masking="PARTIAL", phase_sym=False, phase_hidden=(512, 512), aggregate=False, seed=0,
         widths=None):
    """A single-phase NADE of `depth` amplitude hidden layers on the space of `mol` (LiH, H2O, N2 from the fixtures; "rand30":
    30 qubits, 7 + 7 electrons), default-initialised from `seed`."""
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.nade import NadeMasking
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    from test_nade import ELECTRONS
    N, na, nb = (30, 7, 7) if mol == "rand30" else ELECTRONS[mol]
    hil = Hilbert.get(N, na, nb, encoding=Encoding.SIGNED, make_basis=mol != "rand30")
    torch.manual_seed(seed)
    wf = NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, masking=NadeMasking[masking],
                                   amp_hidden_size=list(widths or [ha] * depth), phase_hidden_size=list(phase_hidden),
                                   use_amp_spin_sym=sym, use_phase_spin_sym=phase_sym, aggregate_phase=aggregate,
                                   n_alpha_electrons=na, n_beta_electrons=nb)
    return hil, wf


def _keys(hil, mol, M, seed=5):
    from test_backward_gpu import _random_keys, _whole_space
    k = _random_keys(hil, M, seed) if mol == "rand30" else _whole_space(hil, seed)[:M]
    return k


def _states(hil, keys):
    return hil.idx2state(torch.as_tensor(np.asarray(keys).astype(np.int64)))


def _kdev(keys):
    return torch.as_tensor(np.asarray(keys).astype(np.int64), device="cuda")


def _expect(ws, M, depth, ha, save=0):
    """naqs_net_last_kernel's phase-kernel part for M rows, with the deep launch in front."""
    import test_forward_f64_gpu as tf
    name = tf._expect("ws" if ws else "h", M, save, {"NAQS_AMP_MODE": "2"}, ha, tf._cus())
    return name.replace(f"amp_mfma_kernel<{ha // 16}>", f"amp_deep_kernel<{ha // 16}, L={depth}>")


def _compare(got, want, P, L):
    got = np.asarray(got, np.float64)
    assert not np.isnan(got).any()
    ninf = ~np.isfinite(want[:, 0])
    assert np.array_equal(ninf, got[:, 0] == -np.inf)
    ok = ~ninf
    d0 = np.abs(got[ok, 0] - want[ok, 0])
    r0 = (d0 / (P * L * LOG_LAYER_PAIR + LOG_REL * np.abs(want[ok, 0]))).max(initial=0.0)
    r1 = np.abs(got[:, 1] - want[:, 1]).max(initial=0.0) / (PHASE_REL * max(PHASE_FLOOR, np.abs(want[:, 1]).max()))
    return r0, r1


# name -> (mol, depth, ha, options, published phase shape (phase_kernel_ws), row counts (cu) -> list)
def _cases():
    import test_forward_f64_gpu as tf
    few = lambda cu: [1, 17, tf.TILE * cu + 1]
    return {
        "rand30_L2_64": ("rand30", 2, 64, {}, True, lambda cu: tf._sizes(tf.WS_RB_CAP, 50000, cu)),
        "rand30_L3_32": ("rand30", 3, 32, {}, True, lambda cu: [1, 17, tf._split_limit(cu) + 1, tf.TILE * cu * 2 + 1, 50000]),
        "rand30_L4_128": ("rand30", 4, 128, {}, False, lambda cu: [1, 17, tf.TILE * cu + 1, 10000]),
        "rand30_L2_64_phasesym": ("rand30", 2, 64, {"phase_sym": True}, False,
                                  lambda cu: tf._sizes(tf.H_RB_CAP[2], 50000, cu)),
        "N2_L2_64": ("N2", 2, 64, {}, True, lambda cu: tf._sizes(tf.WS_RB_CAP, 14400, cu)),
        "N2_L3_128_noampsym": ("N2", 3, 128, {"sym": False}, False, lambda cu: [1, 17, tf.TILE * cu + 1, 14400]),
        "N2_L2_32_nomask": ("N2", 2, 32, {"masking": "NONE"}, True, lambda cu: [17, 10000]),
        "N2_L4_64_fullmask": ("N2", 4, 64, {"masking": "FULL"}, True, lambda cu: [17, 10000]),
        "H2O_L2_64": ("H2O", 2, 64, {}, True, lambda cu: [1, 17, 441]),
        "H2O_L3_32_fullmask_noampsym": ("H2O", 3, 32, {"masking": "FULL", "sym": False}, True, lambda cu: [1, 441]),
        "LiH_L4_32_phasesym": ("LiH", 4, 32, {"phase_sym": True}, False, lambda cu: [1, 17, 225]),
        "LiH_L2_128_nomask_noampsym": ("LiH", 2, 128, {"masking": "NONE", "sym": False}, False, lambda cu: [1, 225]),
    }


@pytest.mark.parametrize("case", list(_cases()))
def test_forward_against_float64(case, capsys):
    from naqs_amd import hamiltonian, packing
    import test_forward_f64_gpu as tf
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    mol, depth, ha, opt, ws, sizes = _cases()[case]
    hil, wf = _net(mol, depth, ha, **opt)
    fused = wf.fused()
    assert fused is not None and fused.amp_depth == depth
    assert fused.n_params == sum(p.numel() for p in wf.model.parameters())
    cu = tf._cus()
    ms = sorted(set(sizes(cu)))
    keys = _keys(hil, mol, max(ms))
    _, w64 = gr.f64_copy(wf)
    want = gr.log_psi_f64(w64, _states(hil, keys))
    P = hil.N // 2
    worst = 0.0
    for M in ms:
        kd = _kdev(keys[:M])
        got = fused.log_psi(kd)
        torch.cuda.synchronize()
        assert fused.last_kernel() == _expect(ws, M, depth, ha), (M, fused.last_kernel())
        r0, r1 = _compare(got.cpu().numpy(), want[:M], P, depth)
        assert r0 <= 1 and r1 <= 1, (case, M, r0, r1)
        worst = max(worst, r0, r1)
        # the training forward: the same launches with SAVE=1, the same bits
        lp2, _ = fused.forward_saved(kd)
        torch.cuda.synchronize()
        assert fused.last_kernel() == _expect(ws, M, depth, ha, save=1), (M, fused.last_kernel())
        assert torch.equal(lp2, got)
    with capsys.disabled():
        print(f"\n[amp depth] {case}: worst error {worst:.2f} x bound over M = {ms}")
    # naqs_logpsi_eloc: the same log psi, the E_loc of ham.local_energy
    if mol != "rand30":
        ham = hamiltonian.DevicePauliHamiltonian(
            packing.load_packed(os.path.join(ROOT, "tests", "golden", f"ham_{mol}.npz")), device="cuda")
        M = max(ms)
        kd = _kdev(np.sort(keys[:M]))
        lp = fused.log_psi(kd)
        lp_e, e = fused.log_psi_and_local_energy(ham, kd)
        torch.cuda.synchronize()
        assert torch.equal(lp, lp_e)
        e_ref = ham.local_energy(kd, lp, kind="log_psi")
        assert torch.equal(e.reshape(e_ref.shape), e_ref)


# -------------------------------------------------------------------------------------------------------------- sampler
def _probs_bound(lp, P):
    """|probs / exp(2 log|psi|) - 1|: both come from the same float32 conditionals — probs as their product (P roundings of
    a value near 1 in relative terms), log|psi| as their float32 sum (P roundings of a partial sum up to |log|psi||, doubled by
    exp(2 .)): 1e-6 + 2 P 2^-24 |log|psi||."""
    return 1e-6 + 2 * P * 2.0 ** -24 * np.abs(lp)


@pytest.mark.parametrize("mol,n,depth", [("LiH", 2_000_000, 2), ("LiH", 2_000_000, 3), ("H2O", 5_000_000, 2),
                                         ("H2O", 5_000_000, 3)])
def test_sampler_distribution(mol, n, depth):
    from scipy import stats
    hil, wf = _net(mol, depth, 64, seed=7)
    fused = wf.fused()
    assert fused is not None
    keys, counts, probs = fused.sample(n, seed=20240607, max_unique=100000)
    assert "sample_expand_deep_kernel<4>" in fused.last_kernel()
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
    assert (rel <= _probs_bound(lp[pos], hil.N // 2)).all(), rel.max()
    obs = np.zeros(len(all_keys))
    obs[pos] = c
    expect = p / p_phys * total
    m = expect >= 5
    chi2 = ((obs[m] - expect[m]) ** 2 / expect[m]).sum() + (obs[~m].sum() - expect[~m].sum()) ** 2 / max(expect[~m].sum(), 1e-9)
    assert stats.chi2.sf(chi2, m.sum()) > 1e-4, (chi2, m.sum())


def test_sampler_same_seed_same_draw():
    hil, wf = _net("rand30", 2, 64, seed=2)
    fused = wf.fused()
    a = fused.sample(10 ** 5, seed=11, max_unique=200000)
    b = fused.sample(10 ** 5, seed=11, max_unique=200000)
    c = fused.sample(10 ** 5, seed=12, max_unique=200000)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not (len(a[1]) == len(c[1]) and torch.equal(a[1], c[1]))
    lp = fused.log_psi(a[0])[:, 0].double()
    rel = (a[2].double() / torch.exp(2 * lp) - 1).abs().cpu().numpy()
    assert (rel <= _probs_bound(lp.cpu().numpy(), hil.N // 2)).all(), rel.max()


# ------------------------------------------------------------------------------------------------------------ gradients
def _grads(wf):
    return {n: p.grad.detach().double().cpu().numpy().copy() for n, p in wf.model.named_parameters()}


def _zero_grad(wf):
    for p in wf.model.parameters():
        p.grad = None


def _grad_cuts():
    from test_backward_gpu import SUMS_FUSE, W0_FUSE, _gin_switch
    import re
    src = open(os.path.join(ROOT, "naqs-for-quantum-chemistry_amd", "csrc", "naqs_amp_deep.hpp")).read()
    dgt = int(re.search(r"constexpr int DGT = (\d+)", src).group(1))
    src = open(os.path.join(ROOT, "naqs-for-quantum-chemistry_amd", "csrc", "naqs_amp_backward.hpp")).read()
    max_wgs = int(re.search(r"constexpr int MAX_TILE_WGS = (\d+)", src).group(1))
    sw = _gin_switch(512)
    return sorted({1, 2, dgt - 1, dgt, dgt + 1, W0_FUSE, W0_FUSE + 1, SUMS_FUSE + 1, dgt * max_wgs, dgt * max_wgs + 1, sw, sw + 1,
                   10000, 50000})


@pytest.mark.parametrize("case", ["rand30_L2_64", "rand30_L3_128_noampsym", "rand30_L4_32_phasesym", "N2_L2_64_fullmask"])
def test_training_step_gradients_against_float64(case, capsys):
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    opts = {"rand30_L2_64": ("rand30", 2, 64, {}), "rand30_L3_128_noampsym": ("rand30", 3, 128, {"sym": False}),
            "rand30_L4_32_phasesym": ("rand30", 4, 32, {"phase_sym": True}),
            "N2_L2_64_fullmask": ("N2", 2, 64, {"masking": "FULL"})}
    mol, depth, ha, opt = opts[case]
    hil, wf = _net(mol, depth, ha, seed=11, **opt)
    fused = wf.fused()
    assert fused is not None and fused.train_mode == "hip"
    cuts = [m for m in _grad_cuts() if m <= (hil.size if mol != "rand30" else 50000)]
    keys = _keys(hil, mol, max(cuts), seed=9)
    _, w64 = gr.f64_copy(wf)
    _, w32 = gr.f64_copy(wf, torch.float32)
    rs = np.random.RandomState(1)
    worst, worst_cpu = 0.0, 0.0
    for M in cuts:
        k = np.sort(keys[:M])
        st = _states(hil, k)
        lp64, margin = gr.log_psi_and_kink_margin(w64, st)
        w = rs.random_sample(M) + 0.1
        w[margin < TAU] = 0.0
        w /= max(w.sum(), 1e-300)
        e = rs.normal(-7.0, 1.0, M) + 1j * rs.normal(0.0, 0.3, M)
        sums = np.array([(w * e.real).sum(), (w * e.imag).sum(), (w * e.real ** 2).sum(), w.sum()])
        # the loss gradient exactly as the device forms it (float32, naqs_grad.hip): what is compared is the backward pass
        g_dev = gr.loss_grad_f32_emulated(e, w, sums).astype(np.float64)
        want = gr.grad_f64(w64, st, g_dev, lp=lp64)
        cpu32 = gr.grad_f64(w32, st.float(), g_dev)
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
        e_d, w_d, s_d = dev(np.stack([e.real, e.imag], -1)), dev(w), dev(sums)
        kd = _kdev(k)
        _zero_grad(wf)
        fused._grad_flat = None
        _, saved = fused.forward_saved(kd)
        fused.backward_from_local_energy(saved, e_d, w_d, s_d)
        g1 = _grads(wf)
        assert "amp_deep_backward_kernel" in fused.last_kernel()
        _zero_grad(wf)
        fused._grad_flat = None
        _, saved = fused.forward_saved(kd)
        g, _ = fused.vmc_loss_grad(e_d, w_d, s_d, with_energy=True)
        fused.backward_saved(saved, g)
        g2 = _grads(wf)
        torch.cuda.synchronize()
        for name in want:
            assert np.array_equal(g1[name], g2[name]), (M, name)
            scale = np.abs(want[name]).max()
            rel = lambda got: np.abs(got - want[name]).max() / scale if scale > 0 else np.abs(got).max()
            err, err32 = rel(g1[name]), rel(cpu32[name])
            assert err <= GRAD_BOUND, (case, M, name, err, err32)
            worst, worst_cpu = max(worst, err), max(worst_cpu, err32)
    with capsys.disabled():
        print(f"\n[amp depth] gradients {case}: worst {worst:.2e} of the tensor scale (float32 autograd on the CPU: {worst_cpu:.2e}) "
              f"over M = {cuts}")


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


@pytest.mark.parametrize("mol,depth", [("N2", 2), ("H2O", 3)])
def test_vmc_run_equals_step_by_step(mol, depth, tmp_path, monkeypatch, capsys):
    """naqs_vmc_run over 20 steps against one naqs_vmc_step per step (test_optimizer_gpu.py does this at depth 1): energies,
    sample counts and parameters bit for bit; and the one-call step against the step-by-step library calls."""
    from naqs_amd.optimizer import LogKey
    runs = {}
    for run, onecall in (("1", "1"), ("0", "1"), ("0", "0")):
        monkeypatch.setenv("NAQS_TRAIN_RUN", run)
        monkeypatch.setenv("NAQS_TRAIN_ONECALL", onecall)
        hil, wf = _net(mol, depth, 64, seed=3)
        opt = _opt(mol, wf, tmp_path / (run + onecall))
        assert wf.fused() is not None
        assert opt._can_onecall() == (onecall == "1") and opt._can_run_in_library() == (run == "1")
        opt.run(n_epochs=20, save_freq=None, save_final=False, output_freq=10)
        out = capsys.readouterr().out
        assert "not available" not in out
        runs[run + onecall] = dict(e=np.array(opt.log[LogKey.E_LOC]), n=np.array(opt.log[LogKey.N_UNIQUE_SAMP]),
                                   p=wf.flatten_parameters().clone(), t=opt.optimizer._t)
    a = runs["11"]
    assert a["t"] == 20 and np.isfinite(a["e"]).all()
    for k in ("01", "00"):
        b = runs[k]
        assert np.array_equal(a["e"], b["e"]) and np.array_equal(a["n"], b["n"]) and torch.equal(a["p"], b["p"]), k


def test_h2o_training_to_convergence_with_two_amplitude_layers(tmp_path, capsys):
    """test_config3_gpu.py's run (the batch script's flags, the default learning-rate schedule, 10 000 steps, seed 111) with
    -n_layer 2: final <E_loc> within 1 mHa of FCI, the sampled-subspace diagonalisation within 0.1 mHa and never below it,
    all on the HIP kernels (no fallback notice)."""
    import json
    import sys
    from conftest import GOLDEN, PKG
    from test_config3_gpu import FLAGS
    sys.path.insert(0, PKG)
    from experiments import _base
    flags = list(FLAGS)
    flags[flags.index("-n_layer") + 1] = "2"
    kat = json.load(open(os.path.join(GOLDEN, "kat.json")))
    res = _base.run(molecule=None, out=None, number=1, lr=-1, n_samps=1e7, n_samps_max=1e12, n_unq_samps_min=1e4,
                    n_unq_samps_max=1e5, n_hid=128, n_layer=1, reweight_samples_by_psi=False, n_train=10000, n_pretrain=0,
                    output_freq=25, save_freq=-1, load_hamiltonian=False, overwrite_hamiltonian=False,
                    presolve_hamiltonian=False, cont=False, n_excitations_max=-1, use_amp_spin_sym=True,
                    use_phase_spin_sym=False, comb_amp_phase=False, aggregate_phase=True, restrict_H=True, reset_opt=False,
                    argv=["-m", os.path.join(GOLDEN, "ham_H2O.npz"), "-o", str(tmp_path / "run"), "-s", "111"] + flags)
    out = capsys.readouterr().out
    r = res[0]
    fci = kat["fci"]["H2O"]
    with capsys.disabled():
        print(f"\n[amp depth] H2O -n_layer 2: final <E_loc> {r['final']:.8f} Ha, subspace {r['eig']:.8f} Ha ({r['n_unq']} states), "
              f"FCI {fci:.8f} Ha, {r['time']:.1f} s for 10 000 steps")
    assert "fused HIP network kernels not available" not in out
    assert -1e-5 < r["final"] - fci < 1e-3, (r["final"], fci)
    assert -1e-8 < r["eig"] - fci < 1e-4, (r["eig"], fci)


def test_published_command_with_two_amplitude_layers_is_fused():
    """The published N2 ansatz with -n_layer 2 gets a fused handle (it fell back to PyTorch modules before)."""
    hil, wf = _net("N2", 2, 64)
    fused = wf.fused()
    assert fused is not None and fused.amp_depth == 2


# ----------------------------------------------------------------------------------------------------------- boundaries
@pytest.mark.parametrize("kind", ["depth5", "mixed", "aggregate"])
def test_outside_the_family_stays_on_torch(kind, capsys):
    if kind == "depth5":
        hil, wf = _net("LiH", 5, 32)
    elif kind == "mixed":
        hil, wf = _net("LiH", 2, 32, widths=[32, 64])
    else:
        hil, wf = _net("LiH", 2, 32, aggregate=True, phase_hidden=(32,))
    assert wf.fused() is None
    out = capsys.readouterr().out
    assert "fused HIP network kernels not available" in out and "amplitude blocks need exactly one hidden layer" in out


def test_create_rejects_bad_depths_and_aggregate():
    import ctypes
    from naqs_amd import _lib
    lib = _lib.load_library()
    hil, wf = _net("LiH", 2, 32)
    fused = wf.fused()
    n = ctypes.c_int64(0)
    assert lib.naqs_net_param_count(fused._h, ctypes.byref(n)) == 0
    assert n.value == sum(p.numel() for p in wf.model.parameters())
    assert lib.naqs_net_amp_param_count(fused._h, ctypes.byref(n)) == 0
    assert n.value == sum(p.numel() for blk in wf.model.amp_layers for p in blk.parameters())
