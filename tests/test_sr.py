"""Natural-gradient training (minSR), the parts that need no GPU: the C-ABI surface of the new entry points, the ``-sr``
switches of the command line, the optimiser's argument, and — in float64 on the PyTorch modules — the two identities the
kernels' design rests on (tests/test_sr_gpu.py holds the kernels to the same reference, tests/sr_reference.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import grad_reference as gr
import sr_reference as sr
from conftest import GOLDEN, PKG, ROOT
from naqs_amd import _lib

torch = pytest.importorskip("torch")
LIH = os.path.join(GOLDEN, "ham_LiH.npz")
NEW = {"naqs_net_sr_gram": 11, "naqs_net_sr_gram_uncentred": 6, "naqs_net_sr_direction": 8}


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "naqs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_lib.lib_path())
    for name, n_args in NEW.items():
        m = re.search(rf"\bint {name}\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n_args, name
        assert hasattr(lib, name), name
    assert "double diag_shift" in code and "M > 32768" in header
    # new entries only: the version every earlier client checks is the library's
    assert int(re.search(r"#define NAQS_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.load_library().naqs_abi_version()


def test_entry_points_refuse_a_null_handle():
    lib = _lib.load_library()
    assert lib.naqs_net_sr_gram(None, 1, None, None, None, 1e-3, None, None, None, None, None) == -1
    assert lib.naqs_net_sr_gram_uncentred(None, 1, None, None, None, None) == -1
    assert lib.naqs_net_sr_direction(None, 1, None, None, None, None, None, None) == -1


def _base():
    sys.path.insert(0, PKG)
    from experiments import _base
    return _base


def test_parser_accepts_sr_and_the_reference_command_lines(monkeypatch, capsys):
    _b = _base()
    p = _b.get_parser(n_hid=128, n_samps=1e7)
    # experiments/bash/naqs/batch_train.sh:14 and the switches of the other published scripts
    a = p.parse_args("-o data/naqs/N2_s111 -m molecules/N2 -single_phase -n1 -n_layer 1 -n_hid 64 -n_layer_phase 2 "
                     "-n_hid_phase 512 -s 111 -n_train 10000 -output_freq 25 -save_freq -1".split())
    assert a.sr is False and (a.molecule, a.n_hid, a.n_hid_phase, a.seed, a.save_freq) == ("molecules/N2", 64, 512, 111, -1)
    a = p.parse_args("-m molecules/N2_1.5 -full_mask_psi -c -r -v".split())
    assert a.sr is False and a.full_mask_psi and a.cont and a.resetOpt and a.verbose
    a = p.parse_args("-m molecules/LiH -single_phase -sr -s 3".split())
    assert a.sr is True and a.single_phase and a.seed == 3 and a.sr_shift > 0 and a.sr_lr > 0
    a = p.parse_args("-m molecules/LiH -sr -sr_shift 1e-4 -sr_lr 0.05 -s 5".split())
    assert a.sr is True and (a.sr_shift, a.sr_lr, a.seed) == (1e-4, 0.05, 5)
    # off: neither the listing nor the call changes; on: the three values travel
    seen = []
    monkeypatch.setattr(_b, "_run", lambda **kw: seen.append(kw) or [])
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7"])
    out = capsys.readouterr().out
    assert "script options:" in out and "sr" not in [ln.split(":")[0].strip() for ln in out.splitlines()] and "sr_shift" not in out
    assert "sr" not in seen[-1] and "sr_lr" not in seen[-1]
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-sr", "-sr_lr", "0.2"])
    out = capsys.readouterr().out
    assert "\tsr : True" in out and "\tsr_lr : 0.2" in out
    assert seen[-1]["sr"] is True and seen[-1]["sr_lr"] == 0.2 and seen[-1]["sr_shift"] == p.get_default("sr_shift")


@pytest.mark.parametrize("argv", [["-comb_amp_phase", "-single_phase"], ["-n_layer", "2"]])
def test_sr_names_the_families_it_does_not_cover(argv, tmp_path):
    _b = _base()
    with pytest.raises(NotImplementedError, match="-sr .natural gradient.: single-phase and aggregate-phase networks with one hidden layer"):
        _b.run(n_hid=16, argv=["-m", LIH, "-o", str(tmp_path / "run"), "-sr", "-s", "7"] + argv)


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
    common = ["-m", LIH, "-o", str(tmp_path / "run"), "-single_phase", "-n_hid", "16", "-n_hid_phase", "32", "-n_train", "2", "-s", "7"]
    with pytest.raises(Reached) as got:
        _b.run(n_hid=128, argv=common)
    assert got.value.args[0] is None
    with pytest.raises(Reached) as got:
        _b.run(n_hid=128, argv=common + ["-sr", "-sr_shift", "1e-4", "-sr_lr", "0.05"])
    assert got.value.args[0] == dict(diag_shift=1e-4, lr=0.05)


def test_optimiser_argument_is_validated_and_switches_the_fused_forms_off():
    from naqs_amd.optimizer import NaturalGradientError, PartialSamplingOptimizer
    assert issubclass(NaturalGradientError, RuntimeError)
    for bad in (dict(diag_shift=0.0, lr=0.1), dict(diag_shift=1e-3, lr=-1.0), dict(diag_shift=1e-3), dict(diag_shift=1e-3, lr=0.1, x=1)):
        with pytest.raises(ValueError, match="natural_gradient"):
            PartialSamplingOptimizer(n_samples=10, natural_gradient=bad)
    opt = object.__new__(PartialSamplingOptimizer)
    opt.use_fused, opt.normalize_grads, opt.bug_compat_full_sample_order, opt.exact_local_energies = True, False, False, False
    opt.natural_gradient = dict(diag_shift=1e-3, lr=0.1)
    assert opt._fused_step_conditions() is False          # no pre-fused sampler call, no one-call step, no in-library run


# ---- the mathematics, float64, PyTorch modules ----------------------------------------------------------------------------
def _hadamard_gram(wf, J):
    """sum over the Linear layers of (Delta Delta^T) o (A A^T + 1) from the Jacobian's own blocks: a layer's bias block is its
    per-sample delta, and its weight block [M, N, K] must be delta_i (x) a_i — a_i is read off it by projection on delta_i, so the
    sum equals J J^T exactly when every per-sample weight gradient is that outer product."""
    named = list(wf.model.named_parameters())
    M = J.shape[0]
    G, off, layers = np.zeros((M, M)), 0, 0
    for (nw, pw), (nb, pb) in zip(named[0::2], named[1::2]):
        assert nw.endswith(".weight") and nb == nw[:-len("weight")] + "bias" and pw.dim() == 2 and pb.shape == pw.shape[:1], (nw, nb)
        N, K = pw.shape
        Jw = J[:, off:off + N * K].reshape(M, N, K)
        off += N * K
        D = J[:, off:off + N]
        off += N
        dd = (D * D).sum(1)
        A = np.einsum("in,ink->ik", D, Jw) / np.where(dd > 0, dd, 1.0)[:, None]
        G += (D @ D.T) * (A @ A.T + 1.0)
        layers += 1
    assert off == J.shape[1]
    return G, layers


def test_hadamard_formula_equals_the_gram_matrix_on_lih():
    """G = A A^T without a Jacobian: LiH, amp_hidden 16, phase [32, 32], float64."""
    case = ("LiH", False, 16, (32, 32), True, "PARTIAL")
    hil, wf = sr.make_net(case, device="cpu")
    _, w64 = gr.f64_copy(wf)
    keys, _ = sr.table(hil, w64, rows=40)
    A, B = sr.jacobians(w64, sr.states_of(hil, keys))
    Ga, layers = _hadamard_gram(w64, A)
    Gp, _ = _hadamard_gram(w64, B)
    assert layers == 2 * 6 + 3
    assert np.abs(A @ A.T).max() > 0 and np.abs(B @ B.T).max() > 0
    assert sr.gram_err(Ga, A @ A.T) < 1e-12 and sr.gram_err(Gp, B @ B.T) < 1e-12


@pytest.mark.parametrize("case", [("LiH", False, 16, (32, 32), True, "PARTIAL"), ("LiH", True, 16, (32,), True, "PARTIAL")],
                         ids=["single", "aggregate"])
def test_amplitude_and_phase_blocks_decouple(case):
    """X_a X_phi^T = 0 in the two supported families: no parameter moves both log|psi| and the phase."""
    hil, wf = sr.make_net(case, device="cpu")
    _, w64 = gr.f64_copy(wf)
    keys, w = sr.table(hil, w64, rows=40)
    A, B = sr.jacobians(w64, sr.states_of(hil, keys))
    assert np.abs(A).max() > 0 and np.abs(B).max() > 0
    assert not np.any((np.abs(A).max(0) > 0) & (np.abs(B).max(0) > 0))
    Xa, Xp = sr.system(A, w, w, 1e-2)[2], sr.system(B, w, w, 1e-2)[2]
    assert np.abs(Xa @ Xp.T).max() == 0.0
    # and the combined family is why it is refused: the last block's first layer moves both
    hil_c, wf_c = gr.sector_net("LiH", device="cpu", amp_hidden=16, phase_hidden=(), combined=True)
    _, wc = gr.f64_copy(wf_c)
    kc, _ = sr.table(hil_c, wc, rows=20)
    Ac, Bc = sr.jacobians(wc, sr.states_of(hil_c, kc))
    assert np.any((np.abs(Ac).max(0) > 0) & (np.abs(Bc).max(0) > 0))


def test_centring_of_the_gram_matrix_is_the_definition():
    """T = D (G - m 1^T - 1 m^T + c) D equals X X^T with X = D (A - 1 w^T A), and sqrt(w) is its null vector (why lambda > 0)."""
    rs = np.random.RandomState(0)
    J = rs.normal(size=(30, 70))
    w = rs.random_sample(30) + 0.1
    w /= w.sum()
    T, _, X = sr.system(J, w, w, 1e-3)
    assert np.allclose(sr.centred(J @ J.T, w, 1e-3), T, rtol=0, atol=1e-12 * np.abs(T).max())
    assert np.abs((X @ X.T) @ np.sqrt(w)).max() < 1e-12 * np.abs(T).max()
