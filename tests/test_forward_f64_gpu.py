"""The log-psi forward on the MI355X against float64 (tests/grad_reference.py), at every kernel form and size class.

naqs_net_logpsi / select_form (naqs_logpsi.hip) picks among phase_kernel_ws<RB, SAVE, SPLIT> (the published shape, amplitude
waves beside the matrix waves), phase_kernel_h<RB, SAVE, FMT> (every other phase shape, the amplitude prologue inside),
phase_kernel<RB> (f32, NAQS_PHASE_MODE=0), the separate amplitude launches (amp_mfma_kernel<2|4|8>, the VALU amp_kernel) and
the aggregate-phase launches (amp2_kernel + agg_finish_kernel, or the unmerged pair).  Each family below runs the row counts
where that choice changes — derived from the source's constants and the device's CU count, not written down — and asserts
the name of what ran (fused.last_kernel()), so a dispatch change that moves a case off its form fails here.

Per case:
* naqs_net_logpsi within the module's bounds of the float64 network (LOG_ABS + LOG_REL |log|psi||; PHASE_REL of the table's
  largest |phase|), -inf exactly where float64 has -inf, no NaN; the worst HIP error is printed beside the error of float32
  PyTorch on the CPU for the same rows;
* the training forward (forward_saved, SAVE=1) gives the same bits (the same kernel, naqs_logpsi.hip);
* naqs_logpsi_eloc gives the same log psi bit for bit, and E_loc bit for bit equal to ham.local_energy of that log psi.
The sampler's probs (fused.sample) are held to exp(2 log|psi|) of float64 — the identity test_grad_reference.py checks for
the torch sampler — and a network trained by the library loop (parameters re-packed inside the step) to the float64 copy of
its current parameters.

Measured on an MI355X, worst HIP error in units of the bound: <= 0.47 in every family (N2 0.32, the 30-qubit nets 0.40-0.47,
the aggregate phase 0.31); the sampler's probs <= 0.12; the trained N2 net 0.47.  Float32 PyTorch on the CPU errs by about
as much (the 30-qubit log|psi|: 2.0e-6 there, 3.4e-6 here).
"""
import math
import os
import re

import numpy as np
import pytest

import grad_reference as gr
from conftest import GOLDEN, ROOT, golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# log|psi| is a sum of P conditional log-amplitudes, each a log-softmax of O(1) logits rounded on its own: the error grows with
# P (P orbital pairs) and with |log|psi||.  N2 (P = 10, |log|psi|| <= 9.3): <= 4.9e-6; the 30-qubit nets (P = 15): ~7e-6.
LOG_PAIR, LOG_REL = 4e-7, 1e-7      # |d log|psi|| <= P LOG_PAIR + LOG_REL |log|psi|_f64|
PHASE_REL, PHASE_FLOOR = 5e-6, 1e-3  # |d phase| <= PHASE_REL * max(PHASE_FLOOR, max |phase_f64| over the table)
U32 = 2.0 ** -24


def _src():
    return open(os.path.join(ROOT, "naqs-for-quantum-chemistry_amd", "csrc", "naqs_logpsi.hip")).read()


def _src_int(pattern):
    return int(re.search(pattern, _src()).group(1))


TILE = _src_int(r"constexpr int BM = RB \* (\d+);")                                   # rows per RB (the MFMA tile)
WS_RB_CAP = _src_int(r"const int rb_ws = std::min\(rb, (\d+)\);")                     # phase_kernel_ws: RB <= 3
H_RB_CAP = {2: _src_int(r"fmt == 2 \? (\d+) : \d+, \(size_t\)"),                      # phase_kernel_h f16x2: RB <= 4
            1: _src_int(r"fmt == 2 \? \d+ : (\d+), \(size_t\)")}                      # ... bf16x3: RB <= 3
F32_RB_CAP = _src_int(r"if \(fmt == 0\) return (\d+);")                               # phase_kernel: RB <= 4
AGG_TILE = _src_int(r"#define NAQS_AMP_TILES (\d+)") * 64                             # amp2_kernel rows per workgroup (x WAVE)
AGG_FIN = _src_int(r"agg_finish_kernel, dim3\(\(unsigned\)\(\(M \+ \d+\) / (\d+)\)\)")        # agg_finish_kernel rows per workgroup


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rb(M, cap, cu):
    return min(cap, max(1, math.ceil(M / (TILE * cu))))


def _split_limit(cu):
    """Largest M of phase_kernel_ws's SPLIT form: two workgroups per 16-row tile, all resident (2 tiles <= CUs)."""
    return TILE * (cu // 2)


def _sizes(rb_cap, top, cu):
    """1, 15, 16, 17; the SPLIT limit and TILE*CU*k (k = 1, 2, 3: where RB steps) -1 / 0 / +1; a ragged count (tile*n + 1)
    inside every RB class up to rb_cap (and one of the SPLIT form); 10 000 (the bench shape); top.  Those <= top."""
    sl = _split_limit(cu)
    m = [1, 15, 16, 17, TILE * (cu // 4) + 1, sl - 1, sl, sl + 1]
    for k in (1, 2, 3):
        m += [TILE * cu * k - 1, TILE * cu * k, TILE * cu * k + 1]
    for rb in range(1, rb_cap + 1):
        n = int(TILE * cu * (rb - 0.25)) // (TILE * rb)
        m.append(TILE * rb * n + 1)
    m += [10000, top]
    return sorted({x for x in m if x <= top})


def _expect(kind, M, save, env, ha, cu):
    """The name naqs_net_last_kernel gives for M rows (select_form / net_logpsi_impl / agg_logpsi of naqs_logpsi.hip)."""
    amp_mode = int(env.get("NAQS_AMP_MODE", "1"))
    amp = "amp_kernel" if amp_mode == 0 else f"amp_mfma_kernel<{ha // 16}>"
    if kind == "agg":
        if amp_mode == 2:
            return f"{amp} + amp_kernel(raw) + agg_finish_kernel"
        if int(env.get("NAQS_AGG_MERGE", "7")) & 1:
            return "amp2_kernel + agg_finish_kernel"
        return "amp_kernel + amp_kernel(raw) + agg_finish_kernel"
    fmt = int(env.get("NAQS_PHASE_MODE", "2"))
    beside = amp_mode == 1 and ha <= 64 and fmt != 0
    if kind == "ws":
        split = env.get("NAQS_WS_SPLIT", "1") != "0" and 2 * math.ceil(M / TILE) <= cu
        rb = 1 if split else _rb(M, WS_RB_CAP, cu)
        return (f"phase_kernel_ws<RB={rb}, SAVE={save}{', SPLIT=1' if split else ''}> (f16x2"
                + (", amplitude waves beside the matrix waves)" if beside else f") + {amp}"))
    if fmt == 0:
        return f"phase_kernel<RB={_rb(M, F32_RB_CAP, cu)}> (f32 MFMA) + {amp}"
    return (f"phase_kernel_h<RB={_rb(M, H_RB_CAP[fmt], cu)}, SAVE={save}, FMT={fmt} ({'f16x2' if fmt == 2 else 'bf16x3'})>"
            + (" incl. amplitude prologue" if beside else f" + {amp}"))


def _bound_log(want, P):
    return P * LOG_PAIR + LOG_REL * np.abs(want)


def _compare(got, want, P):
    """got: HIP (or CPU float32) log psi [m, 2]; want: float64 [m, 2]; P orbital pairs -> (problems, worst |d| log, worst
    |d| phase, worst ratio to the bound)."""
    got = np.asarray(got, np.float64)
    bad = []
    if np.isnan(got).any():
        bad.append("NaN")
    ninf = ~np.isfinite(want[:, 0])
    if not np.array_equal(ninf, got[:, 0] == -np.inf):
        bad.append(f"-inf pattern ({int(ninf.sum())} in float64, {int((got[:, 0] == -np.inf).sum())} here)")
    ok = ~ninf & np.isfinite(got[:, 0])
    d0 = np.abs(got[ok, 0] - want[ok, 0])
    d1 = np.abs(got[:, 1] - want[:, 1])
    b1 = PHASE_REL * max(PHASE_FLOOR, np.abs(want[:, 1]).max())
    r0 = (d0 / _bound_log(want[ok, 0], P)).max(initial=0.0)
    r1 = d1.max(initial=0.0) / b1
    if not r0 <= 1:
        bad.append(f"log|psi| {d0.max():.2e} ({r0:.2f} x bound)")
    if not r1 <= 1:
        bad.append(f"phase {d1.max():.2e} ({r1:.2f} x bound)")
    return bad, d0.max(initial=0.0), d1.max(initial=0.0), max(r0, r1)


def _dev_wf(fix, masking=None):
    from test_nade import make_wf
    from test_variants import split
    try:
        mol = split(fix)[0]
    except ValueError:
        mol = fix
    hil, wf = make_wf(mol, golden(f"nade_{fix}.npz"), device="cuda", masking=masking)
    return mol, hil, wf


def _random_net(amp_hidden=64, phase_sym=False, seed=3):
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    torch.manual_seed(seed)
    hil = Hilbert.get(30, 7, 7, encoding=Encoding.SIGNED)
    wf = NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, amp_hidden_size=[amp_hidden],
                                   phase_hidden_size=[512, 512], use_amp_spin_sym=True, use_phase_spin_sym=phase_sym,
                                   aggregate_phase=False, n_alpha_electrons=7, n_beta_electrons=7)
    return "Li2O", hil, wf


def _unphysical_mix(hil, M, seed):
    """M distinct keys of N2's 20 qubits: 70 % physical (whole-space permutation), 30 % with a wrong electron count."""
    from test_backward_gpu import _whole_space
    rs = np.random.RandomState(seed)
    phys = _whole_space(hil, seed)[: M - M * 3 // 10]
    cand = np.unique(rs.randint(0, 1 << hil.N, size=8 * M).astype(np.uint64))
    cand = cand[~hil.is_physical(cand)]
    keys = np.concatenate([phys, rs.permutation(cand)[: M - len(phys)]])
    assert len(keys) == M and len(np.unique(keys)) == M
    return rs.permutation(keys)


# family -> dict(src, kind, runs=[env, ...], sizes(cu) -> list, eloc sizes, extra runs [(env, sizes)])
def _families():
    def full(cap, top):
        return lambda cu: _sizes(cap, top, cu)

    def per_rb(cap):
        return lambda cu: [TILE * cu * (rb - 1) + TILE * rb * 7 + 1 for rb in range(1, cap + 1)]

    amp_modes = [{"NAQS_AMP_MODE": "1"}, {"NAQS_AMP_MODE": "2"}, {"NAQS_AMP_MODE": "0"}]
    few = lambda cu: [17, _split_limit(cu) + 1, TILE * cu + 1, 10000]
    return {
        # published shape (phase_kernel_ws)
        "N2": dict(src="N2", kind="ws", runs=[{}, {"NAQS_WS_SPLIT": "0"}], sizes=full(WS_RB_CAP, 14400),
                   eloc=lambda cu: [17, _split_limit(cu), TILE * cu + 1, 10000]),
        "N2_phase1.5": dict(src="N2", scale_phase=1.5, kind="ws", runs=[{}, {"NAQS_WS_SPLIT": "0"}],
                            sizes=full(WS_RB_CAP, 14400), eloc=lambda cu: [10000]),
        "rand30_512": dict(src="rand", kind="ws", runs=[{}, {"NAQS_WS_SPLIT": "0"}], sizes=full(WS_RB_CAP, 50000),
                           eloc=lambda cu: [50000]),
        # other phase shapes (phase_kernel_h), the bf16x3 and f32 formats
        "LiH": dict(src="LiH", kind="h", runs=[{}], sizes=lambda cu: [1, 15, 16, 17, 100, 225], eloc=lambda cu: [225]),
        "H2O": dict(src="H2O", kind="h", runs=[{}], sizes=lambda cu: [1, 17, 441], eloc=lambda cu: [441]),
        "N2_nomask": dict(src="N2_nomask", kind="h", runs=[{}], sizes=full(H_RB_CAP[2], 14400), eloc=lambda cu: [10000]),
        "rand30_phasesym": dict(src="rand", phase_sym=True, kind="h", runs=[{}], sizes=full(H_RB_CAP[2], 50000),
                                eloc=lambda cu: [50000],
                                extra=[({"NAQS_PHASE_MODE": "1"}, per_rb(H_RB_CAP[1])),
                                       ({"NAQS_PHASE_MODE": "0"}, per_rb(F32_RB_CAP))]),
        # amplitude widths (the prologue / waves beside for 32 and 64; amp_mfma_kernel<2|4|8>; the VALU amp_kernel)
        "rand30_amp32": dict(src="rand", amp_hidden=32, kind="ws", runs=amp_modes, sizes=few, eloc=lambda cu: []),
        "rand30_amp64": dict(src="rand", amp_hidden=64, seed=4, kind="ws", runs=amp_modes, sizes=few, eloc=lambda cu: []),
        "rand30_amp128": dict(src="rand", amp_hidden=128, kind="h", runs=amp_modes, sizes=few, eloc=lambda cu: [10000]),
        # aggregate phase: merged (amp2_kernel), unmerged VALU and unmerged matrix-core amplitude blocks
        "N2_aggphase": dict(src="N2_aggphase", kind="agg",
                            runs=[{}, {"NAQS_AGG_MERGE": "0"}, {"NAQS_AMP_MODE": "2"}],
                            sizes=lambda cu: sorted({1, 17, AGG_TILE - 1, AGG_TILE, AGG_TILE + 1, AGG_FIN - 1, AGG_FIN, AGG_FIN + 1,
                                                     2 * AGG_TILE + 1, 10000, 14400}),
                            eloc=lambda cu: [AGG_TILE + 1, 14400]),
        "LiH_phasesym_agg": dict(src="LiH_phasesym_agg", kind="agg", runs=[{}, {"NAQS_AGG_MERGE": "0"}, {"NAQS_AMP_MODE": "2"}],
                                 sizes=lambda cu: [1, 17, 225], eloc=lambda cu: [225]),
        # masking
        "N2_2.25_fullmask": dict(src="N2_2.25_fullmask", kind="ws", runs=[{}], sizes=lambda cu: [17, 2049, 10000],
                                 eloc=lambda cu: [10000]),
        "CH2_noampsym": dict(src="CH2_noampsym", kind="h", runs=[{}], sizes=lambda cu: [1, 17, 735], eloc=lambda cu: [735]),
        "N2_fullmask_unphysical": dict(src="N2_2.25_fullmask", unphysical=True, kind="ws", runs=[{}, {"NAQS_WS_SPLIT": "0"}],
                                       sizes=lambda cu: [17, _split_limit(cu), 10000], eloc=lambda cu: []),
    }


def _build(fam):
    if fam["src"] == "rand":
        mol, hil, wf = _random_net(fam.get("amp_hidden", 64), fam.get("phase_sym", False), fam.get("seed", 3))
    else:
        mol, hil, wf = _dev_wf(fam["src"])
    if fam.get("scale_phase"):
        with torch.no_grad():
            for p in wf.model.phase_layers.parameters():
                p.mul_(fam["scale_phase"])
    return mol, hil, wf


def _set_env(monkeypatch, env, keys=("NAQS_AMP_MODE", "NAQS_AGG_MERGE", "NAQS_WS_SPLIT", "NAQS_PHASE_MODE")):
    for k in keys:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("family", list(_families()))
def test_forward_against_float64_at_every_form(family, monkeypatch):
    from naqs_amd import hamiltonian, packing
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    fam = _families()[family]
    cu = _cus()
    mol, hil, wf = _build(fam)
    ha = wf.model.amp_layers[0].linears()[0].out_features
    P = hil.N // 2
    fused = wf.fused()
    assert fused is not None
    runs = [(env, fam["sizes"](cu)) for env in fam["runs"]] + [(env, s(cu)) for env, s in fam.get("extra", [])]
    eloc_sizes = fam["eloc"](cu)
    M = max([max(s) for _, s in runs] + eloc_sizes)
    if fam.get("unphysical"):
        keys = _unphysical_mix(hil, M, 5)
    else:
        from test_backward_gpu import _random_keys, _whole_space
        keys = _random_keys(hil, M, 5) if fam["src"] == "rand" else _whole_space(hil, 5)[:M]
    assert len(keys) == M, (family, len(keys), M)
    # the float64 and float32 references, once, on the largest key set
    states = hil.idx2state(torch.as_tensor(keys.astype(np.int64)))
    _, wf64 = gr.f64_copy(wf)
    _, wf32 = gr.f64_copy(wf, dtype=torch.float32)
    ref64 = gr.log_psi_f64(wf64, states)
    ref32 = gr.log_psi_f64(wf32, states)
    assert not np.isnan(ref64).any()
    if fam.get("unphysical"):
        assert (~np.isfinite(ref64[:, 0])).sum() >= M // 5

    fails, worst = [], 0.0
    for env, sizes in runs:
        _set_env(monkeypatch, env)
        if "NAQS_PHASE_MODE" in env:
            fused.refresh()                                  # (the number format is chosen when the weights are packed)
        for m in sizes:
            ks, want, want32 = gr.sorted_rows(keys, m, ref64, ref32)
            k_d = torch.as_tensor(ks.astype(np.int64), device="cuda")
            lp = fused.log_psi(k_d).clone()
            name = fused.last_kernel()
            exp_name = _expect(fam["kind"], m, 0, env, ha, cu)
            torch.cuda.synchronize()
            bad, e0, e1, r = _compare(lp.cpu().numpy(), want, P)
            _, c0, c1, _ = _compare(want32, want, P)
            worst = max(worst, r)
            if name != exp_name:
                bad.append(f"ran {name!r}, expected {exp_name!r}")
            saved = "-"
            if env.get("NAQS_PHASE_MODE") != "0":            # (the f32 kernel saves no activations: no training forward)
                lpt, _ = fused.forward_saved(k_d)
                name_t = fused.last_kernel()
                exp_t = _expect(fam["kind"], m, 1, env, ha, cu)
                saved = "same bits" if torch.equal(lpt, lp) else "DIFFERENT"
                if not torch.equal(lpt, lp):
                    bad.append("forward_saved differs from naqs_net_logpsi")
                if name_t != exp_t:
                    bad.append(f"training forward ran {name_t!r}, expected {exp_t!r}")
            print(f"[forward {family} {env or 'default'}] M={m:6d} {name}  |HIP - f64| log {e0:.2e} phase {e1:.2e} "
                  f"({r:.2f} x bound)  |torch f32 CPU - f64| log {c0:.2e} phase {c1:.2e}  training forward: {saved}")
            fails += [(m, str(env), b) for b in bad]
    _set_env(monkeypatch, {})
    if any("NAQS_PHASE_MODE" in env for env, _ in runs):
        fused.refresh()

    if eloc_sizes:
        ham = hamiltonian.DevicePauliHamiltonian(packing.load_packed(os.path.join(GOLDEN, f"ham_{mol}.npz")), device="cuda:0")
        for m in eloc_sizes:
            ks, want = gr.sorted_rows(keys, m, ref64)
            k_d = torch.as_tensor(ks.astype(np.int64), device="cuda")
            lp = fused.log_psi(k_d).clone()
            lp2, e2 = fused.log_psi_and_local_energy(ham, k_d)
            e_ref = ham.local_energy(k_d, lp2, kind="log_psi")
            torch.cuda.synchronize()
            same_lp, same_e = torch.equal(lp2, lp), torch.equal(e2, e_ref)
            print(f"[forward+E_loc {family}] M={m:6d} {fused.last_kernel()}  log psi {'same bits' if same_lp else 'DIFFERENT'}, "
                  f"E_loc {'same bits' if same_e else 'DIFFERENT'} as ham.local_energy")
            if not (same_lp and same_e and torch.isfinite(e2).all()):
                fails.append(("eloc", m, same_lp, same_e))
            bad, _, _, r = _compare(lp2.cpu().numpy(), want, P)
            worst = max(worst, r)
            fails += [("eloc", m, b) for b in bad]
    print(f"[forward {family}] worst HIP error {worst:.2f} x bound")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ the sampler's probs
SAMPLE_CASES = [("N2", 500, "1"), ("N2", 5000, "1"), ("N2", 1_000_000, "1"), ("N2", 5000, "0"), ("N2", 1_000_000, "0"),
                ("rand30", 1_000_000, "1"), ("rand30", 1_000_000, "0"), ("N2_noampsym", 1_000_000, "1"), ("N2_aggphase", 1_000_000, "1")]


@pytest.mark.parametrize("src,n,mfma", SAMPLE_CASES)
def test_sampler_probs_against_float64(src, n, mfma, monkeypatch):
    """probs of every unique sample within 2 (log|psi| bound) + 8 P 2^-24 (P float32 products of conditionals) relative of
    exp(2 log|psi|_f64) — the identity test_sampler_probs_are_psi_squared_in_float64 checks for the torch sampler."""
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    monkeypatch.setenv("NAQS_SAMPLE_MFMA", mfma)
    if src == "rand30":
        mol, hil, wf = _random_net()
    else:
        mol, hil, wf = _dev_wf(src)
    fused = wf.fused()
    keys, counts, probs = fused.sample(n, seed=20261016, max_unique=1 << 20)
    k = keys.cpu().numpy().astype(np.uint64)
    p = probs.double().cpu().numpy()
    assert len(k) > 50 and np.all(np.diff(k) > 0) and hil.is_physical(k).all()
    if src == "rand30":
        assert len(k) > 20000
    states = hil.idx2state(torch.as_tensor(k.astype(np.int64)))
    _, wf64 = gr.f64_copy(wf)
    _, wf32 = gr.f64_copy(wf, dtype=torch.float32)
    lp64 = gr.log_psi_f64(wf64, states)[:, 0]
    lp32 = gr.log_psi_f64(wf32, states)[:, 0]
    want = np.exp(2 * lp64)
    P = hil.N // 2
    bound = 2 * _bound_log(lp64, P) + 8 * P * U32
    rel = np.abs(p / want - 1)
    rel32 = np.abs(np.exp(2 * lp32) / want - 1)
    print(f"[sampler {src} n={n} NAQS_SAMPLE_MFMA={mfma}] {len(k)} unique  |probs / exp(2 log|psi|_f64) - 1| {rel.max():.2e} "
          f"({(rel / bound).max():.2f} x bound)  torch f32 CPU exp(2 log|psi|): {rel32.max():.2e}")
    assert np.all(rel <= bound), (rel.max(), (rel / bound).max())


# ------------------------------------------------------------------------------------------------ a trained network
@pytest.mark.parametrize("overlap", ["2", "1", "0"])
def test_forward_after_library_training_steps(overlap, tmp_path, monkeypatch):
    """N2 trained for 200 steps by PartialSamplingOptimizer.run on the library loop, which re-packs the parameters inside
    each step (NAQS_PACK_OVERLAP: 2 the next sampler launch hosts the whole re-pack, 1 the phase share only, 0 in order):
    with no refresh in between, the forward at the SPLIT / RB=1 / RB=3 sizes is held to the float64 copy of the CURRENT
    parameters.  (test_pending_phase_repack_is_finished_by_whoever_comes_next makes the modes agree with each other; this
    catches a stale layer common to all of them.)"""
    from test_backward_gpu import _whole_space
    from test_optimizer_gpu import make_opt_gpu
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    monkeypatch.setenv("NAQS_PACK_OVERLAP", overlap)
    z, hil, wf, opt = make_opt_gpu("N2", tmp_path)
    assert opt._can_onecall()
    p0 = wf.flatten_parameters().clone()
    opt.run(n_epochs=200, save_freq=None, save_final=False, output_freq=10 ** 9)
    torch.cuda.synchronize()
    fused = wf._fused                                      # (not wf.fused(): no refresh from the version counters)
    assert fused is not None and fused is not False
    assert not torch.equal(wf.flatten_parameters(), p0)
    _, wf64 = gr.f64_copy(wf)
    cu = _cus()
    sizes = [_split_limit(cu), TILE * cu, 10000]
    keys = _whole_space(hil, 5)[:max(sizes)]
    ref64 = gr.log_psi_f64(wf64, hil.idx2state(torch.as_tensor(keys.astype(np.int64))))
    fails = []
    for m in sizes:
        ks, want = gr.sorted_rows(keys, m, ref64)
        lp = fused.log_psi(torch.as_tensor(ks.astype(np.int64), device="cuda"))
        name = fused.last_kernel()
        exp_name = _expect("ws", m, 0, {}, 64, cu)
        bad, e0, e1, r = _compare(lp.cpu().numpy(), want, hil.N // 2)
        print(f"[trained N2 NAQS_PACK_OVERLAP={overlap}] M={m:6d} {name}  |HIP - f64| log {e0:.2e} phase {e1:.2e} ({r:.2f} x bound)")
        if name != exp_name:
            bad.append(f"ran {name!r}, expected {exp_name!r}")
        fails += [(m, b) for b in bad]
    assert not fails, fails
