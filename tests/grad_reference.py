"""The float64 reference of the training backward (a plain helper module, like oracle_backend.py).

The PyTorch formulation of the network (naqs_amd.nade) follows the dtype of its parameters, so a float64 copy of a network
on the CPU is an exact-arithmetic stand-in for what the HIP backward computes in float32:

* ``f64_copy``                 the same network, on the CPU, in float64 (or any other dtype);
* ``log_psi_and_kink_margin``  log psi plus, per row, the smallest |input| of any ReLU — rows whose margin is within
                               rounding of zero may take the other branch in float32 (a different, equally valid gradient);
* ``grad_f64``                 d/d theta sum_i g_i . log psi_i per parameter name;
* ``loss_grad_f64`` / ``loss_grad_f32_emulated``
                               d loss / d (log|psi|, phase) of the VMC loss of _SGD_step (energy.py:328-329): exactly, and in
                               the float32 arithmetic vmc_grad_kernel documents (naqs_grad.hip);
* ``kink_free``                g with the rows near a kink zeroed;
* ``log_psi_f64``              the forward alone, in chunks of rows (no graph): float64 numpy [M, 2];
* ``sorted_rows``              the first m rows of a key set in the library's (ascending) order, with their reference rows.
"""
import contextlib

import numpy as np
import torch
from torch import nn

from conftest import golden


def f64_copy(src, dtype=torch.float64):
    """``src``: a ``nade_<fixture>.npz`` name (``"N2_aggphase"``) or a ``NAQSComplex_NADE_orbitals`` on any device ->
    (hilbert, the same network on the CPU in ``dtype``)."""
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    if isinstance(src, str):
        from test_nade import make_wf
        from test_variants import split
        try:
            mol = split(src)[0]
        except ValueError:                  # a base fixture: nade_<mol>.npz
            mol = src
        hil, wf = make_wf(mol, golden(f"nade_{src}.npz"))
    else:
        m = src.model
        lin = m.phase_layers[0].linears() if len(m.phase_layers) else []
        wf = NAQSComplex_NADE_orbitals(
            src.hilbert, qubit_ordering=[int(q) for q in src.qubit2model_permutation], masking=m.masking,
            amp_hidden_size=[l.out_features for l in m.amp_layers[0].linears()[:-1]],
            phase_hidden_size=[l.out_features for l in lin[:-1]], use_amp_spin_sym=m.use_amp_spin_sym,
            use_phase_spin_sym=m.use_phase_spin_sym, aggregate_phase=m.aggregate_phase,
            combined_amp_phase_blocks=m.combined_amp_phase_blocks,
            n_alpha_electrons=m.n_alpha_up if m.use_restricted_hilbert else None,
            n_beta_electrons=m.n_beta_up if m.use_restricted_hilbert else None, device="cpu")
        wf.model.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
        hil = src.hilbert
    wf.model.to(dtype)
    return hil, wf


@contextlib.contextmanager
def _relu_inputs(model, sink):
    """Record min |x| over each row of every ReLU input while the block is active: forward pre-hooks on the nn.ReLU modules
    (the single phase MLP) and a wrapper around torch.relu (the amplitude blocks and the per-pair phase blocks, nade.py)."""
    def note(x):
        sink.append(x.detach().abs().reshape(x.shape[0], -1).amin(1))

    hooks = [mod.register_forward_pre_hook(lambda mod, args: note(args[0])) for mod in model.modules()
             if isinstance(mod, nn.ReLU)]
    relu = torch.relu

    def wrapped(x, *a, **k):
        note(x)
        return relu(x, *a, **k)

    torch.relu = wrapped
    try:
        yield
    finally:
        torch.relu = relu
        for h in hooks:
            h.remove()


def log_psi_and_kink_margin(wf, states):
    """states: [M, N] (+-1, qubit order) -> (log psi [M, 2] with its autograd graph, margin float64 numpy [M]: the smallest
    |pre-activation| of any ReLU the row passes through)."""
    mins = []
    with _relu_inputs(wf.model, mins):
        lp = wf.log_psi(states).reshape(-1, 2)
    M = lp.shape[0]
    margin = torch.full((M,), float("inf"), dtype=torch.float64)
    for m in mins:
        margin = torch.minimum(margin, m.double())
    return lp, margin.numpy()


def grad_f64(wf, states, g, lp=None):
    """{parameter name: d/d theta sum_i g[i] . log psi_i} as float64 numpy arrays (float64 network: exact to ~1e-15); ``lp``:
    a log psi of these states with its graph, when the caller already has one."""
    if lp is None:
        lp = wf.log_psi(states).reshape(-1, 2)
    names, params = zip(*wf.model.named_parameters())
    g = torch.as_tensor(np.asarray(g), dtype=lp.dtype).reshape(-1, 2)
    grads = torch.autograd.grad((lp * g).sum(), params, allow_unused=True)
    return {n: (np.zeros(tuple(p.shape)) if d is None else d.double().numpy()) for n, p, d in zip(names, params, grads)}


def loss_grad_f64(eloc, w):
    """d loss / d (log|psi|, phase) of loss = 2 Re sum_i w_i log psi_i (E_i - <E>)^*, <E> = sum_i w_i E_i (energy.py:328-329),
    in float64.  eloc: complex [M] or float [M, 2]; w: [M] -> [M, 2]."""
    e = _complex(eloc)
    w = np.asarray(w, np.float64)
    d = e - (w * e).sum()
    return np.stack([2 * w * d.real, -2 * w * d.imag], -1)


def loss_grad_f32_emulated(eloc, w, sums):
    """vmc_grad_kernel's arithmetic (naqs_grad.hip): g = (((float)Re E - (float)sums[0]) * (2 (float)w),
    -(((float)Im E - (float)sums[1]) * (2 (float)w))), every operation rounded to float32."""
    e = _complex(eloc)
    f = np.float32
    two_w = f(2.0) * np.asarray(w, np.float64).astype(f)
    m_re, m_im = f(sums[0]), f(sums[1])
    return np.stack([(e.real.astype(f) - m_re) * two_w, -((e.imag.astype(f) - m_im) * two_w)], -1)


def kink_free(g, margin, tau=1e-5):
    """g with the rows whose margin is below tau zeroed -> (g, number of rows zeroed)."""
    g = np.array(g, copy=True)
    near = np.asarray(margin) < tau
    g[near] = 0
    return g, int(near.sum())


def _complex(eloc):
    e = np.asarray(eloc)
    if np.iscomplexobj(e):
        return e.astype(np.complex128)
    return e[..., 0].astype(np.float64) + 1j * e[..., 1].astype(np.float64)


def log_psi_f64(wf, states, chunk=4096):
    """log psi [M, 2] of ``states`` ([M, N] +-1, qubit order) through the network ``wf`` (an ``f64_copy``: float64, or float32
    for the CPU float32 error it is compared with), as float64 numpy.  The forward is row-independent: chunks of rows give
    the same numbers as one pass and bound the memory of the [512, 512] networks."""
    states = torch.as_tensor(states)
    out = np.empty((states.shape[0], 2), np.float64)
    with torch.no_grad():
        for lo in range(0, states.shape[0], chunk):
            out[lo:lo + chunk] = wf.log_psi(states[lo:lo + chunk]).reshape(-1, 2).double().numpy()
    return out


def sorted_rows(keys, m, *tables):
    """keys: the key set a reference was computed on, in its own order; -> (its first m keys ascending — the order the
    library's tables are kept in —, then each table's rows in that order)."""
    order = np.argsort(keys[:m], kind="stable")
    return (keys[:m][order],) + tuple(t[:m][order] for t in tables)
