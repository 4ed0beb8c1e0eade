"""Natural gradient with momentum (SPRING), the parts that need no GPU: the C-ABI surface of ``naqs_net_sr_jvp``, the
``momentum`` key of the optimiser's argument, the ``-sr_momentum`` switch, the float64 definitions of tests/spring_reference.py
and — on the float64 PyTorch modules — the identity the Jacobian-vector kernel rests on:

    (J v)_i = sum over the Linear layers l of  delta_l,i . (V_l a_l,i + v_b,l)

with a_l,i the layer's input and delta_l,i the gradient of the output's row i, taken with hooks during one forward and one
backward pass, and V_l / v_b,l the slices of v that are the layer's weight / bias (tests/test_sr_momentum_gpu.py holds the
kernel to the same float64 Jacobians)."""
import contextlib
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import grad_reference as gr
import spring_reference as spring
import sr_reference as sr
from conftest import GOLDEN, PKG, ROOT
from naqs_amd import _lib

torch = pytest.importorskip("torch")
LIH = os.path.join(GOLDEN, "ham_LiH.npz")
SHIFT = 1e-2


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_jvp_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "naqs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint naqs_net_sr_jvp\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 7
    assert "const float *v_dev" in m.group(1) and "double *ua_dev" in m.group(1) and "double *uphi_dev" in m.group(1)
    res, args = _lib.SIGNATURES["naqs_net_sr_jvp"]
    assert res is ctypes.c_int and len(args) == 7
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "naqs_net_sr_jvp")
    # an addition: the version every earlier client checks is unchanged
    assert int(re.search(r"#define NAQS_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.load_library().naqs_abi_version() == 9


def test_jvp_entry_point_refuses_a_null_handle():
    assert _lib.load_library().naqs_net_sr_jvp(None, 1, None, None, None, None, None) == -1


# ---- the optimiser's argument and the command line ----------------------------------------------------------------------
def test_momentum_key_is_validated():
    from naqs_amd.optimizer import PartialSamplingOptimizer
    base = dict(diag_shift=1e-3, lr=0.1)
    for bad in (1.0, 1.5, -0.1, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match=r"natural_gradient: .*momentum"):
            PartialSamplingOptimizer(n_samples=10, natural_gradient=dict(base, momentum=bad))
    with pytest.raises(ValueError, match="natural_gradient"):
        PartialSamplingOptimizer(n_samples=10, natural_gradient=dict(base, momentum=0.5, x=1))
    with pytest.raises(ValueError, match="natural_gradient"):
        PartialSamplingOptimizer(n_samples=10, natural_gradient=dict(lr=0.1, momentum=0.5))
    # the accepted forms get past the check (and fail later, on the arguments this call leaves out)
    for good in (0, 0.0, 0.5, 0.99, np.float64(0.9)):
        for more in ({}, dict(solver="hip")):
            with pytest.raises(Exception) as got:
                PartialSamplingOptimizer(n_samples=10, natural_gradient=dict(base, momentum=good, **more))
            assert "natural_gradient" not in str(got.value)


def test_momentum_step_calls_the_jvp_only_with_a_previous_step():
    """``_natural_gradient_update`` on stand-ins: mu = 0 or absent never calls ``sr_jvp`` and keeps no step; mu > 0 takes the plain
    step first, then solves for y - mu sqrt(w) o (u - w^T u) and adds mu phi_prev."""
    from naqs_amd.optimizer import PartialSamplingOptimizer
    eye = torch.eye(3, dtype=torch.float64)
    w = torch.tensor([0.2, 0.3, 0.5], dtype=torch.float64)

    class Fused:
        def __init__(self):
            self.calls = []

        def sr_gram(self, saved, w, g, shift):
            return 4 * eye, 16 * eye, torch.ones(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)

        def sr_jvp(self, saved, v):
            self.calls.append(("jvp", v.tolist()))
            return torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64), torch.tensor([0.0, 0.0, 4.0], dtype=torch.float64)

        def sr_direction(self, saved, w, xa, xp):
            self.calls.append(("dir", xa.tolist(), xp.tolist()))
            return torch.ones(2)

    class Wf:
        def __init__(self):
            self.p = torch.zeros(2)

        def flatten_parameters(self):
            return self.p

    for ng in (dict(diag_shift=1e-3, lr=0.1), dict(diag_shift=1e-3, lr=0.1, momentum=0.0)):
        opt = object.__new__(PartialSamplingOptimizer)
        opt.natural_gradient, opt.wavefunction = ng, Wf()
        fused = Fused()
        for _ in range(2):
            opt._natural_gradient_update(fused, None, w, None)
        assert [c[0] for c in fused.calls] == ["dir", "dir"] and getattr(opt, "_sr_phi_prev", None) is None
        assert opt.sr_last["momentum"] == 0.0 and "jvp_norm" not in opt.sr_last
        assert torch.allclose(opt.wavefunction.p, torch.full((2,), -0.2))

    mu = 0.5
    opt = object.__new__(PartialSamplingOptimizer)
    opt.natural_gradient, opt.wavefunction = dict(diag_shift=1e-3, lr=0.1, momentum=mu), Wf()
    fused = Fused()
    opt._natural_gradient_update(fused, None, w, None)
    assert fused.calls == [("dir", [0.25] * 3, [0.0625] * 3)] and "jvp_norm" not in opt.sr_last
    assert torch.equal(opt._sr_phi_prev, torch.ones(2)) and torch.equal(opt.wavefunction.p, torch.full((2,), -0.1))
    opt._natural_gradient_update(fused, None, w, None)
    assert fused.calls[1] == ("jvp", [1.0, 1.0])
    wn, ua, up = w.numpy(), np.array([1.0, 2.0, 3.0]), np.array([0.0, 0.0, 4.0])
    ra = 1.0 - mu * np.sqrt(wn) * (ua - wn @ ua)
    rp = 1.0 - mu * np.sqrt(wn) * (up - wn @ up)
    assert fused.calls[2][0] == "dir"
    assert np.allclose(fused.calls[2][1], ra / 4, rtol=1e-15, atol=0) and np.allclose(fused.calls[2][2], rp / 16, rtol=1e-15, atol=0)
    assert torch.equal(opt._sr_phi_prev, torch.full((2,), 1.5)) and opt.sr_last["momentum"] == mu
    assert float(opt.sr_last["jvp_norm"]) == pytest.approx(np.sqrt(1 + 4 + 9 + 16))
    assert torch.allclose(opt.wavefunction.p, torch.full((2,), -0.25))


def _base():
    sys.path.insert(0, PKG)
    from experiments import _base
    return _base


def test_parser_accepts_sr_momentum_and_lists_it_only_when_given(monkeypatch, capsys):
    _b = _base()
    p = _b.get_parser(n_hid=128)
    assert p.parse_args("-m molecules/LiH -sr".split()).sr_momentum == 0
    assert p.parse_args("-m molecules/LiH -sr -sr_momentum 0.9".split()).sr_momentum == 0.9
    seen = []
    monkeypatch.setattr(_b, "_run", lambda **kw: seen.append(kw) or [])
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-sr"])
    assert "sr_momentum" not in capsys.readouterr().out and "sr_momentum" not in seen[-1]
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-sr", "-sr_momentum", "0.9"])
    assert "\tsr_momentum : 0.9" in capsys.readouterr().out and seen[-1]["sr_momentum"] == 0.9 and seen[-1]["sr"] is True


def test_sr_momentum_without_sr_is_refused(tmp_path):
    _b = _base()
    with pytest.raises(ValueError, match="-sr_momentum .* -sr"):
        _b.run(n_hid=16, argv=["-m", LIH, "-o", str(tmp_path / "run"), "-s", "7", "-sr_momentum", "0.9"])
    with pytest.raises(ValueError, match="-sr_momentum .* -sr"):
        _b._run(**dict.fromkeys(
            ("molecule_fname hamiltonian_fname exp_name num_experiments pretrained_model_loc continue_experiment reset_optimizer "
             "qubit_ordering masking lr lr_lut n_samps n_samps_max n_unq_samps_min n_unq_samps_max reweight_samples_by_psi n_train "
             "n_pretrain output_freq save_freq n_lut n_hid n_layer n_hid_phase n_layer_phase n_excitations_max comb_amp_phase "
             "use_amp_spin_sym use_phase_spin_sym aggregate_phase use_restrictedH loadH presolveH overwrite_pauli_hamiltonian verbose "
             "seed").split()), sr_momentum=0.5)


def test_switch_reaches_the_optimiser(tmp_path, monkeypatch):
    import oracle_backend
    _b = _base()
    oracle_backend.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    class Reached(Exception):
        pass

    def grab(**kw):
        raise Reached(kw.get("natural_gradient"))

    monkeypatch.setattr(_b, "PartialSamplingOptimizer", grab)
    common = ["-m", LIH, "-o", str(tmp_path / "run"), "-single_phase", "-n_hid", "16", "-n_hid_phase", "32", "-n_train", "2", "-s", "7",
              "-sr", "-sr_shift", "1e-4", "-sr_lr", "0.05"]
    with pytest.raises(Reached) as got:
        _b.run(n_hid=128, argv=common)
    assert got.value.args[0] == dict(diag_shift=1e-4, lr=0.05)
    with pytest.raises(Reached) as got:
        _b.run(n_hid=128, argv=common + ["-sr_momentum", "0.9", "-sr_solver", "hip"])
    assert got.value.args[0] == dict(diag_shift=1e-4, lr=0.05, solver="hip", momentum=0.9)


# ---- the mathematics, float64 ----------------------------------------------------------------------------------------------
_TAB = {}


def _table(case, rows=40):
    if case not in _TAB:
        hil, wf = sr.make_net(case, device="cpu")
        _, w64 = gr.f64_copy(wf)
        keys, w = sr.table(hil, w64, rows=rows)
        states = sr.states_of(hil, keys)
        A, B = sr.jacobians(w64, states)
        rs = np.random.RandomState(7)
        e = rs.normal(-7.0, 1.0, len(keys)) + 1j * rs.normal(0.0, 0.3, len(keys))
        _TAB[case] = dict(w64=w64, states=states, w=w, A=A, B=B, g=gr.loss_grad_f64(e, w))
    return _TAB[case]


@pytest.mark.parametrize("case", [sr.CASES[4], sr.CASES[6]], ids=sr.case_id)
def test_spring_direction_is_the_plain_one_at_zero_and_stationary_above(case):
    t = _table(case)
    A, B, w, g = t["A"], t["B"], t["w"], t["g"]
    d = sr.direction(A, B, w, g, SHIFT)
    prev = np.random.RandomState(3).normal(size=A.shape[1])
    assert np.array_equal(spring.spring_direction(A, B, w, g, SHIFT, 0.0, prev), d)
    assert np.array_equal(spring.spring_direction(A, B, w, g, SHIFT, 0.9, None), d)
    for mu, pv in ((0.5, prev), (0.9, d), (0.99, prev)):
        phi = spring.spring_direction(A, B, w, g, SHIFT, mu, pv)
        res = spring.stationarity(A, B, w, g, SHIFT, mu, pv, phi)
        assert res <= 1e-10, (case, mu, res)
        # a step that is not the minimiser does not pass: the plain direction shifted by mu phi_prev
        assert spring.stationarity(A, B, w, g, SHIFT, mu, pv, mu * pv + d) > 1e-4


@contextlib.contextmanager
def _linear_taps(model, taps):
    """Hooks on every Linear layer of the network while it runs: ``taps`` receives (weights, biases, input, output) per layer call,
    the output with ``retain_grad`` so that the backward pass leaves delta on it.  The phase MLP runs as nn.Linear modules
    (forward hooks); the per-pair blocks run stacked, layer by layer, through torch.einsum("bnk,nhk->bnh") (a wrapper)."""
    def keep(mod, args, out):
        out.retain_grad()
        taps.append(("mlp", mod, args[0], out))

    hooks = [lin.register_forward_hook(keep) for blk in (model.phase_layers if not model.aggregate_phase else []) for lin in blk.linears()]
    einsum = torch.einsum

    def wrapped(eq, *ops):
        out = einsum(eq, *ops)
        if eq == "bnk,nhk->bnh":
            out.retain_grad()
            taps.append(("blocks", None, ops[0], out))
        return out

    torch.einsum = wrapped
    try:
        yield
    finally:
        torch.einsum = einsum
        for h in hooks:
            h.remove()


def _jvp_from_layers(wf, states, v):
    """(A v, B v) from the layers' inputs and output gradients alone."""
    model = wf.model
    off, where = 0, {}
    for _, p in model.named_parameters():
        where[id(p)] = (off, p.numel())
        off += p.numel()
    v = torch.as_tensor(v, dtype=torch.float64)

    def piece(p):
        o, n = where[id(p)]
        return v[o:o + n].reshape(p.shape)

    taps = []
    with _linear_taps(model, taps):
        lp = wf.log_psi(states).reshape(-1, 2)
    P = len(model.amp_layers)
    n_lin = len(model.amp_layers[0].linears())
    sets = [model.amp_layers] + ([model.phase_layers] if model.aggregate_phase else [])
    stacked = [k for k, t in enumerate(taps) if t[0] == "blocks"]
    assert len(stacked) == n_lin * len(sets) and len(taps) - len(stacked) == (0 if model.aggregate_phase else len(model.phase_layers[0].linears()))
    out = []
    for c in range(2):
        for t in taps:
            t[3].grad = None
        lp[:, c].sum().backward(retain_graph=True)
        u = torch.zeros(lp.shape[0], dtype=torch.float64)
        for k, (kind, mod, a, y) in enumerate(taps):
            if y.grad is None:
                continue                                   # (the other component's layers)
            delta = y.grad
            if kind == "mlp":
                u += (delta * (a @ piece(mod.weight).t() + piece(mod.bias))).sum(-1)
                continue
            blocks, l = sets[stacked.index(k) // n_lin], stacked.index(k) % n_lin
            W = a.shape[-1] // 2
            for n in range(P):
                lin = blocks[n].linears()[l]
                if l > 0:
                    an = a[:, n]
                else:                                      # the first layer's padded inputs: pair n reads n of each half, pair 0 one (zero)
                    an = a[:, n, :1] if n == 0 else torch.cat([a[:, n, :n], a[:, n, W:W + n]], -1)
                u += (delta[:, n] * (an @ piece(lin.weight).t() + piece(lin.bias))).sum(-1)
        out.append(u.detach().numpy())
    return out


@pytest.mark.parametrize("case", [("LiH", False, 16, (32, 32), True, "PARTIAL"), ("LiH", True, 16, (32,), True, "PARTIAL")],
                         ids=["single", "aggregate"])
def test_jvp_is_a_sum_over_layers_of_delta_times_layer_of_v(case):
    t = _table(case)
    A, B = t["A"], t["B"]
    v = np.random.RandomState(5).normal(size=A.shape[1])
    ua, up = _jvp_from_layers(t["w64"], t["states"], v)
    wa, wp = spring.jvp64(A, B, v)
    assert np.abs(wa).max() > 0 and np.abs(wp).max() > 0
    assert spring.jvp_err(ua, A, v) < 1e-13 and spring.jvp_err(up, B, v) < 1e-13
    # one tensor at a time: a layer paired with another layer's slice of v fails
    off = 0
    for name, p in t["w64"].model.named_parameters():
        e = np.zeros_like(v)
        e[off:off + p.numel()] = v[off:off + p.numel()]
        off += p.numel()
        ua, up = _jvp_from_layers(t["w64"], t["states"], e)
        assert spring.jvp_err(ua, A, e) < 1e-13 and spring.jvp_err(up, B, e) < 1e-13, name
