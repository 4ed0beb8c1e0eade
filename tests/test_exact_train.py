"""Training on exact local energies, the parts that need no GPU: the command-line switch and its way to the optimiser, the
constructor's refusal of the full-sample quirk, the distribution policy, and the binding's signature table
(tests/test_exact_train_gpu.py holds the library call and the step to their definitions on the MI355X)."""
import ctypes
import os
import sys

import pytest
import torch

from conftest import GOLDEN, PKG
from test_optimizer import make_opt

LIH = os.path.join(GOLDEN, "ham_LiH.npz")


def _base():
    sys.path.insert(0, PKG)
    from experiments import _base
    return _base


def test_switch_parses_and_is_hidden_from_the_listing_when_off(monkeypatch, capsys):
    _b = _base()
    p = _b.get_parser(n_hid=128)
    assert p.parse_args(["-m", LIH]).train_exact_eloc is False
    assert p.parse_args(["-m", LIH, "-train_exact_eloc"]).train_exact_eloc is True
    assert "Train on exact local energies (psi on every connected state)" in " ".join(p.format_help().split())
    seen = []
    monkeypatch.setattr(_b, "_run", lambda **kw: seen.append(kw) or [])
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7"])
    out = capsys.readouterr().out
    assert "script options:" in out and "train_exact_eloc" not in out and "exact_eloc" not in out
    assert seen[-1]["train_exact_eloc"] is False and seen[-1]["exact_eloc"] is False
    _b.run(n_hid=128, argv=["-m", LIH, "-o", "unused", "-s", "7", "-train_exact_eloc"])
    out = capsys.readouterr().out
    assert "\ttrain_exact_eloc : True" in out and "\texact_eloc :" not in out
    assert seen[-1]["train_exact_eloc"] is True and seen[-1]["exact_eloc"] is False


@pytest.mark.parametrize("on", [False, True])
def test_switch_reaches_the_optimiser(on, tmp_path, monkeypatch):
    import oracle_backend
    _b = _base()
    oracle_backend.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    class Reached(Exception):
        pass

    def grab(**kw):
        raise Reached(kw.get("exact_local_energies"))

    monkeypatch.setattr(_b, "PartialSamplingOptimizer", grab)
    with pytest.raises(Reached) as got:
        _b.run(n_hid=128, argv=["-m", LIH, "-o", str(tmp_path / "run"), "-single_phase", "-n_hid", "16", "-n_hid_phase", "32",
                                "-n_layer_phase", "2", "-n_train", "2", "-s", "7"] + (["-train_exact_eloc"] if on else []))
    assert got.value.args[0] is on


def test_constructor_refuses_the_full_sample_quirk(tmp_path, monkeypatch):
    with pytest.raises(NotImplementedError, match="exact local energies with bug_compat_full_sample_order: the quirk reorders the table"):
        make_opt("LiH", tmp_path, monkeypatch, exact_local_energies=True, bug_compat_full_sample_order=True)
    # each of the two alone is accepted, and the switch is stored on the base class
    _, _, _, opt = make_opt("LiH", tmp_path, monkeypatch, exact_local_energies=True)
    assert opt.exact_local_energies is True and opt.n_connected == []
    _, _, _, opt = make_opt("LiH", tmp_path, None, bug_compat_full_sample_order=True)
    assert opt.exact_local_energies is False
    _, _, _, opt = make_opt("LiH", tmp_path, None)
    assert opt.exact_local_energies is False


def test_exact_mode_takes_no_fused_step_form(tmp_path, monkeypatch):
    _, _, _, opt = make_opt("LiH", tmp_path, monkeypatch, exact_local_energies=True)
    assert not opt._fused_step_conditions() and not opt._can_prefuse() and not opt._can_onecall() and not opt._can_shard_onecall()


class _Group:
    """torch.distributed as the policy sees it: a world of four, this process rank 0."""
    @staticmethod
    def get_world_size():
        return 4

    @staticmethod
    def get_rank():
        return 0


def test_distribution_policy_stays_replicated_in_exact_mode(tmp_path, monkeypatch, capsys):
    from naqs_amd import optimizer as O
    monkeypatch.setattr(O, "_dist", lambda: _Group)
    for exact, want in ((True, "replicated"), (False, "sharded")):
        _, _, _, opt = make_opt("LiH", tmp_path, monkeypatch if exact else None, exact_local_energies=exact)
        opt.shard_min_rows, opt.shard_min_table = 1, 8
        for M in (4, 10 ** 4, 10 ** 6):                # far beyond shard_min_table: a truncated step would shard
            opt._last_M = M
            mode = opt._choose_dist_mode(trust_local=True)
            assert mode == (want if M >= 8 else "replicated"), (exact, M, mode)
        opt.shard_min_rows = 0                          # "forces sharding" — not in exact mode
        assert opt._choose_dist_mode(trust_local=True) == want
        assert (opt._active_dist() is None) == exact
    capsys.readouterr()


def test_signature_table_carries_the_entry_point():
    from naqs_amd import _lib
    res, args = _lib.SIGNATURES["naqs_exact_eloc"]
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert res is ctypes.c_int
    assert args == [vp, vp, i64, vp, vp, i64, i64, i64, vp, vp, vp, ctypes.POINTER(i64), vp]
    assert _lib.ABI_VERSION == 9
    header = open(os.path.join(os.path.dirname(PKG), "include", "naqs_hip.h")).read()
    assert "int naqs_exact_eloc(naqs_net_t *net, naqs_ham_t *ham, int64_t M, uint64_t *keys_dev, float *logpsi_dev," in header
