"""Deep amplitude blocks without a GPU: the binding of naqs_net_create_amp_layers, its argument checks (made before any
device is touched) and the flat parameter layout it documents, against the PyTorch module's state_dict."""
import ctypes

import pytest

from naqs_amd import _lib

torch = pytest.importorskip("torch")

OK, INVALID, UNSUPPORTED = 0, -1, -4


def _cfg(n_qubits=12, amp_hidden=64, aggregate=0):
    cfg = _lib.NetConfig()
    cfg.n_qubits = n_qubits
    cfg.n_alpha, cfg.n_beta = 2, 2
    cfg.masking = 1
    cfg.use_amp_spin_sym = 1
    cfg.amp_hidden = amp_hidden
    cfg.n_phase_hidden = 1
    cfg.phase_hidden[0] = 64
    for i in range(n_qubits):
        cfg.qubit2model[i] = i
    cfg.aggregate_phase = aggregate
    return cfg


def _create(cfg, depth):
    lib = _lib.load_library()
    h = ctypes.c_void_p(None)
    st = lib.naqs_net_create_amp_layers(ctypes.byref(cfg) if cfg is not None else None, depth, 0, ctypes.byref(h))
    assert h.value is None           # nothing is created on any of the paths tested here
    return st


def test_binding():
    res, args = _lib.SIGNATURES["naqs_net_create_amp_layers"]
    assert res is ctypes.c_int and args[1] is ctypes.c_int32 and len(args) == 4
    assert _lib.NET_MAX_AMP_LAYERS == 4


@pytest.mark.parametrize("depth", [0, -1, 5, 100])
def test_depth_outside_one_to_four_is_invalid(depth):
    assert _create(_cfg(), depth) == INVALID


def test_null_config_is_invalid():
    assert _create(None, 2) == INVALID


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_aggregate_phase_with_deep_blocks_is_unsupported(depth):
    assert _create(_cfg(aggregate=1), depth) == UNSUPPORTED


@pytest.mark.parametrize("width", [200, 40, 144])
def test_other_widths_are_unsupported(width):
    assert _create(_cfg(amp_hidden=width), 2) == UNSUPPORTED


def _pair_floats(ha, nout, L, n):
    """naqs_amp_deep.hpp: deep_pair_floats."""
    nin = 1 if n == 0 else 2 * n
    return ha * nin + ha + (L - 1) * (ha * ha + ha) + nout * ha + nout


@pytest.mark.parametrize("depth,ha,sym", [(2, 64, True), (3, 32, False), (4, 128, True)])
def test_flat_layout_is_the_state_dict_block_by_block(depth, ha, sym):
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    hil = Hilbert.get(20, 7, 7, encoding=Encoding.SIGNED)
    wf = NAQSComplex_NADE_orbitals(hil, device="cpu", qubit_ordering=-1, amp_hidden_size=[ha] * depth,
                                   phase_hidden_size=[512, 512], use_amp_spin_sym=sym, aggregate_phase=False,
                                   n_alpha_electrons=7, n_beta_electrons=7)
    names = [n for n, _ in wf.model.named_parameters()]
    sizes = dict(wf.model.named_parameters())
    nout = 5 if sym else 4
    off = 0
    for n in range(10):
        want = [f"amp_layers.{n}.layers.{l}.0.{k}" for l in range(depth + 1) for k in ("weight", "bias")]
        assert names[2 * (depth + 1) * n: 2 * (depth + 1) * (n + 1)] == want
        got = sum(sizes[w].numel() for w in want)
        assert got == _pair_floats(ha, nout, depth, n)
        off += got
    assert off == sum(p.numel() for blk in wf.model.amp_layers for p in blk.parameters())
    assert names[2 * (depth + 1) * 10].startswith("phase_layers.0.")
