"""Qubit orderings other than the default -1 (``-qo``, experiments/_base.py:35), on the CPU: the torch formulation.

A ``qubit2model`` list q2m says which qubit (key bit) model position i reads.  The contract held here and on the device
(test_qubit_ordering_gpu.py): spin-preserving pair permutations (model pair n is orbital pair pi(n): alpha on even, beta on odd
model positions); the network is a function of the model-order occupations alone, so the same parameters on relabelled keys
give the same wave function; and the sampler emits its table in (prefix, outcome) order of the MODEL pairs — ascending keys
only at -1.  Orderings that swap alpha and beta inside a pair are outside the contract (the reference's own state2shell
assumes alpha on even model positions).

* invariance in float64: every ansatz form of the device suite at ordering +1 and at a seeded pair permutation, against the
  -1 network with the same state_dict on the relabelled whole space: log psi to 1e-12, the same -inf rows under FULL masking;
* the torch sampler at those orderings: model_index strictly increasing, physical keys, counts against the exact
  probabilities (test_nade.test_sampler_statistics' seed, draw count and statistic, plus a chi-square at p > 1e-4);
* the helpers themselves (relabel_keys / model_index / pair_ordering) against direct statements of what they compute.
The reference's own vectors at +1 (nade_LiH_qo1.npz) run through test_variants.py.
"""
import numpy as np
import pytest
import torch
from scipy import stats

import grad_reference as gr

# every handle family of the device suite: (sector_net arguments)
FORMS = {
    "ws": dict(amp_hidden=64, phase_hidden=(512, 512)),
    "h": dict(phase_hidden=(32, 32)),
    "h_phasesym": dict(phase_hidden=(32, 32), phase_sym=True),
    "agg": dict(aggregate=True, phase_hidden=(64,)),
    "agg_phasesym": dict(aggregate=True, phase_hidden=(64,), phase_sym=True),
    "comb": dict(combined=True, amp_hidden=64),
    "deep": dict(amp_layers=3, amp_hidden=32),
    "aggdeep": dict(aggregate=True, amp_layers=2, amp_hidden=32, phase_hidden=(32, 32)),
    "full": dict(masking="FULL"),
}
ORDERINGS = ["+1", "pi"]
PV = 1e-4


def ordering(tag, P):
    """"+1" -> 1; "pi" -> pair_ordering(P, seed=1) (a qubit2model list)."""
    return 1 if tag == "+1" else gr.pair_ordering(P, seed=1)


def chi2_pvalue(obs, p):
    """Counts against probabilities over the same states: cells of >= 5 expected draws, the rest pooled -> (chi2, cells, p)."""
    expect = p / p.sum() * obs.sum()
    m = expect >= 5
    chi2 = ((obs[m] - expect[m]) ** 2 / expect[m]).sum()
    cells = int(m.sum())
    if (~m).any():
        chi2 += (obs[~m].sum() - expect[~m].sum()) ** 2 / max(expect[~m].sum(), 1e-9)
        cells += 1
    return chi2, cells, stats.chi2.sf(chi2, cells - 1)


def _whole(hil):
    return np.sort(hil.restricted2full_idx(np.arange(hil.size)).astype(np.uint64))


def _states(hil, keys):
    return hil.idx2state(torch.as_tensor(np.asarray(keys).astype(np.int64)))


def test_helpers_state_what_they_compute():
    P = 6
    q_m1, q_p1, q_pi = gr.q2m_of(-1, 2 * P), gr.q2m_of(1, 2 * P), gr.pair_ordering(P, 1)
    assert q_m1 == [10, 11, 8, 9, 6, 7, 4, 5, 2, 3, 0, 1] and q_p1 == list(range(12))
    pi = [q // 2 for q in q_pi[0::2]]
    assert sorted(pi) == list(range(P)) and pi != list(range(P)) and pi != list(range(P))[::-1]
    assert all(q_pi[2 * n] == 2 * pi[n] and q_pi[2 * n + 1] == 2 * pi[n] + 1 for n in range(P))
    assert gr.pair_ordering(P, 1) == q_pi and gr.pair_ordering(16, 1) != gr.pair_ordering(16, 2)
    rs = np.random.RandomState(0)
    keys = rs.randint(0, 1 << 12, size=300).astype(np.uint64)
    for qf, qt in ((q_m1, q_p1), (q_m1, q_pi), (q_pi, q_p1)):
        out = gr.relabel_keys(keys, qf, qt)
        for k, o in zip(keys.tolist()[:50], out.tolist()[:50]):
            assert all((k >> qf[i]) & 1 == (o >> qt[i]) & 1 for i in range(12))
        assert np.array_equal(gr.relabel_keys(out, qt, qf), keys)
        assert np.array_equal(gr.model_index(out, qt), gr.model_index(keys, qf))
    # at -1 the model index IS the key: pair 0 on the top bits, alpha + 2 beta = the pair's two key bits
    assert np.array_equal(gr.model_index(keys, q_m1), keys.astype(np.int64))
    # 32-bit keys: bits 30 / 31 travel to pair 0 at -1 and to pair 15 at +1
    top = np.array([1 << 31, 1 << 30], np.uint64)
    assert gr.model_index(top, gr.q2m_of(-1, 32)).tolist() == [2 * 4 ** 15, 4 ** 15]
    assert gr.model_index(top, gr.q2m_of(1, 32)).tolist() == [2, 1]
    assert gr.relabel_keys(top, gr.q2m_of(-1, 32), gr.q2m_of(1, 32)).tolist() == [2, 1]


@pytest.mark.parametrize("tag", ORDERINGS)
@pytest.mark.parametrize("name", ["LiH", "syn10_3_2"])
@pytest.mark.parametrize("form", list(FORMS))
def test_relabelling_invariance_in_float64(form, name, tag):
    """The network at ordering O on the whole space against the -1 network with the same state_dict on the relabelled keys."""
    N = gr.sector(name)[1]
    O = ordering(tag, N // 2)
    hil, wfA = gr.sector_net(name, device="cpu", seed=3, **FORMS[form])
    _, wfB = gr.sector_net(name, device="cpu", seed=4, qubit_ordering=O, **FORMS[form])
    wfB.model.load_state_dict(wfA.model.state_dict())
    _, A64 = gr.f64_copy(wfA)
    _, B64 = gr.f64_copy(wfB)
    qA, qB = gr.q2m_of(-1, N), gr.q2m_of(O, N)
    assert [int(q) for q in wfA.qubit2model_permutation] == qA and [int(q) for q in wfB.qubit2model_permutation] == qB
    assert [int(q) for q in B64.qubit2model_permutation] == qB                   # (f64_copy carries the ordering over)
    kB = _whole(hil)
    if form == "full":                                                            # -inf rows: wrong electron counts
        bad = np.arange(1 << N, dtype=np.uint64)
        bad = bad[~hil.is_physical(bad)]
        kB = np.concatenate([kB, np.random.RandomState(2).permutation(bad)[:hil.size // 3]])
    kA = gr.relabel_keys(kB, qB, qA)
    assert np.array_equal(hil.is_physical(kA), hil.is_physical(kB))               # pair permutations keep the sector
    assert not np.array_equal(kA, kB)
    lpB = gr.log_psi_f64(B64, _states(hil, kB))
    lpA = gr.log_psi_f64(A64, _states(hil, kA))
    assert not np.isnan(lpA).any() and not np.isnan(lpB).any()
    infA, infB = ~np.isfinite(lpA[:, 0]), ~np.isfinite(lpB[:, 0])
    assert np.array_equal(infA, infB)
    if form == "full":
        assert np.array_equal(infB, ~hil.is_physical(kB)) and infB.sum() >= hil.size // 4
    else:
        assert not infB.any()
    d = np.abs(lpA[~infA] - lpB[~infB]).max()
    assert d <= 1e-12, d
    # the relabelling matters: the ordering-O network on the UNrelabelled keys is another function
    assert np.abs(gr.log_psi_f64(B64, _states(hil, kA[:hil.size]))[:, 0] - lpA[:hil.size, 0]).max() > 1e-3


@pytest.mark.parametrize("tag", ORDERINGS)
def test_torch_sampler_at_other_orderings(tag):
    """wavefunction.sample through the torch modules at ordering O: (prefix, outcome) order, physical unique keys, and the
    counts against the exact |psi|^2 over the whole space (seed, draw count and z-score bounds of
    test_nade.test_sampler_statistics; a chi-square on top)."""
    O = ordering(tag, 6)
    hil, wf = gr.sector_net("LiH", device="cpu", seed=3, qubit_ordering=O, phase_hidden=(32, 32))
    q = gr.q2m_of(O, 12)
    g = torch.Generator().manual_seed(7)
    n = 400000
    states, counts, probs, lp = wf.sample(n, generator=g)
    keys = hil.state2idx(states).squeeze().numpy().astype(np.uint64)
    assert np.all(np.diff(gr.model_index(keys, q)) > 0)                     # unique, in (prefix, outcome) order
    assert not np.all(np.diff(keys.astype(np.int64)) > 0)                   # ... which is not ascending key order here
    assert hil.is_physical(keys).all()
    assert counts.dtype == torch.int64 and 0 < counts.sum().item() <= n
    assert np.allclose(probs.numpy(), lp[:, 0].detach().exp().pow(2).numpy(), rtol=2e-4, atol=1e-9)
    all_keys = _whole(hil)
    _, wf64 = gr.f64_copy(wf)
    p_all = np.exp(2 * gr.log_psi_f64(wf64, _states(hil, all_keys))[:, 0])
    kept = counts.sum().item()
    assert abs(kept / n - p_all.sum()) < 5 * np.sqrt(p_all.sum() * (1 - p_all.sum()) / n) + 1e-3
    pos = np.searchsorted(all_keys, keys)
    assert np.array_equal(all_keys[pos], keys)
    freq = np.zeros(len(all_keys))
    freq[pos] = counts.numpy()
    expect = p_all * n
    big = expect > 50
    z = (freq[big] - expect[big]) / np.sqrt(expect[big])
    assert np.abs(z).max() < 6 and abs(z.mean()) < 0.5
    chi2, cells, pv = chi2_pvalue(freq, p_all)
    print(f"[torch sampler LiH {tag}] {len(keys)} unique, kept {kept} of {n}; chi2 {chi2:.1f} over {cells} cells, p-value {pv:.3g}")
    assert pv > PV, (chi2, cells, pv)
