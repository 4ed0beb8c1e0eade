"""Combined amplitude-phase blocks with a single phase (``-single_phase -comb_amp_phase``) without a GPU: the PyTorch modules
against the reference's vectors (tests/golden/make_golden_comb.py), their float64 copy against the recorded loss and gradients
(the float64 reference test_comb_amp_phase_gpu.py holds the HIP kernels to), and the argument checks of
naqs_net_create_combined, made before any device is touched."""
import ctypes

import numpy as np
import pytest
import torch

import grad_reference as gr
from conftest import golden
from naqs_amd import _lib

FIXTURES = [("LiH", "LiH_single"), ("LiH", "LiH_nosym"), ("N2", "N2_single")]
OK, INVALID, UNSUPPORTED = 0, -1, -4


def _wf(mol, fix):
    from test_nade import make_wf
    z = golden(f"comb_{fix}.npz")
    hil, wf = make_wf(mol, z)
    return z, hil, wf


@pytest.mark.parametrize("mol,fix", FIXTURES)
def test_fixture_is_the_single_phase_combined_ansatz(mol, fix):
    z, _, wf = _wf(mol, fix)
    m = wf.model
    sym = bool(z["cfg_use_amp_spin_sym"])
    assert m.combined_amp_phase_blocks and not m.aggregate_phase and len(m.phase_layers) == 0
    assert m.use_phase_spin_sym == m.use_amp_spin_sym == sym            # (the constructor makes the phase symmetry follow)
    na, nph = (5, 3) if sym else (4, 4)
    for n, blk in enumerate(m.amp_layers):
        lin = blk.linears()
        assert len(lin) == 2 and lin[0].in_features == max(1, 2 * n) and lin[0].out_features == 64
        assert lin[1].out_features == (na + nph if n == m.P - 1 else na)


@pytest.mark.parametrize("mol,fix", FIXTURES)
def test_modules_reproduce_reference_conditionals_and_log_psi(mol, fix):
    z, _, wf = _wf(mol, fix)
    s = torch.tensor(z["eval_states"])
    with torch.no_grad():
        cond = wf._evaluate_log_psi(s, gather_state=False).numpy()
        lp = wf.log_psi(s).numpy()
    ref = z["eval_cond"]
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(cond))                       # the masked outcomes: -inf in both
    assert np.max(np.abs(cond[fin] - ref[fin])) < 2e-5
    assert np.max(np.abs(lp - z["eval_log_psi"])) < 5e-5
    # the phase comes from the last model block only: one pair's phase column is nonzero, every other one is zero
    assert np.count_nonzero(np.any(cond[..., 1] != 0, axis=(0, 2))) == 1


@pytest.mark.parametrize("mol,fix", FIXTURES)
def test_f64_modules_reproduce_reference_loss_and_gradients(mol, fix):
    """The ragged branch of _forward_predict in float64 (grad_reference.f64_copy) against the reference's _SGD_step: sgd_loss and
    grad:* to 2e-3 of each tensor's scale (the reference ran in float32)."""
    z, _, wf32 = _wf(mol, fix)
    _, wf = gr.f64_copy(wf32)
    assert all(p.dtype == torch.float64 for p in wf.model.parameters())
    s = torch.tensor(z["samp_states"])
    lp, margin = gr.log_psi_and_kink_margin(wf, s)
    assert np.max(np.abs(lp.detach().numpy() - z["samp_log_psi"])) < 5e-5 and np.all(margin >= 0)
    w = z["samp_counts"].astype(np.float64)
    w /= w.sum()
    e = z["sgd_eloc_c128"]
    d = e - (w * e).sum()
    loss = 2 * (torch.as_tensor(w) * (lp[:, 0] * torch.as_tensor(d.real) - lp[:, 1] * torch.as_tensor(d.imag))).sum()
    assert abs(loss.item() - float(z["sgd_loss"])) < 1e-4 * max(1, abs(float(z["sgd_loss"])))
    got = gr.grad_f64(wf, s, gr.loss_grad_f64(e, w), lp=lp)
    last = f"amp_layers.{wf.model.P - 1}.layers.1.0."
    for name, _ in wf.model.named_parameters():
        g_ref = z["grad:" + name]
        scale = max(1e-3, np.abs(g_ref).max())
        assert np.max(np.abs(got[name] - g_ref)) < 2e-3 * scale, (name, np.max(np.abs(got[name] - g_ref)) / scale)
    # the phase rows of the last block carry gradient (the phase part of the loss reaches them)
    na = 5 if wf.model.use_amp_spin_sym else 4
    assert np.abs(got[last + "weight"][na:]).max() > 0 and np.abs(z["grad:" + last + "weight"][na:]).max() > 0


def _cfg(n_qubits=12, amp_hidden=64, aggregate=0, sym=1, psym=None):
    cfg = _lib.NetConfig()
    cfg.n_qubits = n_qubits
    cfg.n_alpha, cfg.n_beta = 2, 2
    cfg.masking = 1
    cfg.use_amp_spin_sym = sym
    cfg.use_phase_spin_sym = sym if psym is None else psym
    cfg.amp_hidden = amp_hidden
    cfg.n_phase_hidden = 0                         # (ignored)
    for i in range(n_qubits):
        cfg.qubit2model[i] = i
    cfg.aggregate_phase = aggregate
    return cfg


def _create(cfg):
    lib = _lib.load_library()
    h = ctypes.c_void_p(None)
    st = lib.naqs_net_create_combined(ctypes.byref(cfg) if cfg is not None else None, 0, ctypes.byref(h))
    assert h.value is None           # nothing is created on any of the paths tested here
    return st


def test_binding():
    res, args = _lib.SIGNATURES["naqs_net_create_combined"]
    assert res is ctypes.c_int and len(args) == 3 and args[1] is ctypes.c_int


def test_null_config_is_invalid():
    assert _create(None) == INVALID


@pytest.mark.parametrize("sym", [0, 1])
def test_aggregate_phase_is_unsupported(sym):
    assert _create(_cfg(aggregate=1, sym=sym)) == UNSUPPORTED


@pytest.mark.parametrize("width", [200, 40, 144, 8])
def test_other_widths_are_unsupported(width):
    assert _create(_cfg(amp_hidden=width)) == UNSUPPORTED


@pytest.mark.parametrize("sym,psym", [(1, 0), (0, 1)])
def test_phase_symmetry_other_than_the_amplitude_symmetry_is_invalid(sym, psym):
    assert _create(_cfg(sym=sym, psym=psym)) == INVALID


@pytest.mark.parametrize("sym", [True, False])
def test_flat_layout_is_the_state_dict_with_the_phase_rows_in_the_last_block(sym):
    """What naqs_net_create_combined documents: block by block in state_dict order, the last block's output layer
    n_out_amp + n_out_phase rows (amplitude rows first), no phase layers."""
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    hil = Hilbert.get(20, 7, 7, encoding=Encoding.SIGNED)
    wf = NAQSComplex_NADE_orbitals(hil, device="cpu", qubit_ordering=-1, amp_hidden_size=[64], phase_hidden_size=[512, 512],
                                   use_amp_spin_sym=sym, use_phase_spin_sym=sym, aggregate_phase=False,
                                   combined_amp_phase_blocks=True, n_alpha_electrons=7, n_beta_electrons=7)
    names = [n for n, _ in wf.model.named_parameters()]
    sizes = dict(wf.model.named_parameters())
    na, nph = (5, 3) if sym else (4, 4)
    off = 0
    for n in range(10):
        want = [f"amp_layers.{n}.layers.{l}.0.{k}" for l in range(2) for k in ("weight", "bias")]
        assert names[4 * n: 4 * (n + 1)] == want
        nout = na + nph if n == 9 else na
        nin = max(1, 2 * n)
        assert [tuple(sizes[w].shape) for w in want] == [(64, nin), (64,), (nout, 64), (nout,)]
        off += sum(sizes[w].numel() for w in want)
    assert len(names) == 40 and off == sum(p.numel() for p in wf.model.parameters())
