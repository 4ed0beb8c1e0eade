"""The network, sampler and E_loc kernels against float64 at every orbital-pair count P = 2..16 the library accepts.

The other float64 suites run networks of P = 6, 7, 10 and 15 pairs.  Code that branches on P or on the electron sector lives
below and above those: the sampler without a head launch (P <= 4) and with one level after it (P = 5), the hosted re-pack of
the first pairs (P <= 4), full 16-bit alpha and beta strings in the sampler's prefix word and bit 31 of a 32-bit key (P = 16),
the electron budgets at 1 and 9 of 10 orbitals, and the Hamiltonians no other test packs.  One sector per P
(grad_reference.SECTORS: the reference's molecule where one exists, a marked synthetic sector otherwise); networks are
default-initialised from fixed seeds in the published shape, with variants (run.py's aggregate phase, -phase_sym, FULL and
NONE masking, two amplitude layers) at P = 2, 4, 5, 13 and 16.

* forward: fused.log_psi within the bounds of test_forward_f64_gpu.py of the float64 copy (log|psi|: P 4e-7 + 1e-7 |log|psi||,
  x L with L amplitude layers; phase: 5e-6 of the table's largest |phase|), the kernel name, the training forward's bits,
  naqs_logpsi_eloc's bits;
* backward: both training-step call forms bit for bit, each tensor within 2e-5 of its scale of the float64 gradient;
* sampler: probs against exp(2 log|psi|_f64); an exact chi-square over the whole space (P <= 14); a level-by-level
  multinomial test of every tree node (P = 7, 15, 16, FULL masking); each with a host-side power check; every launch cut
  draws the same bits;
* every kind of handle (single phase, deep single phase, aggregate, deep aggregate, combined) with 16-unit blocks of 5 and 3
  outputs at P = 2 and 3, where every per-pair offset of the packed copies is rounded: forward, backward, sampler probs;
* the library's training loop at P <= 5;
* E_loc of every Hamiltonian the reference ships against the oracle, the chunk length each handle derives, and 32-bit keys.

Measured on an MI355X (the whole module: 40 s): worst HIP error 0.45 of the bound in the forward (P = 16), 0.18 in the
backward, 0.10 in the sampler's probs; exact chi-square p-values 0.010 .. 0.91, level-by-level 0.024 .. 0.47.  Power: the
exact chi-square rejects a root share moved down to 3e-4 .. 1e-2 (1e-2 at P = 13, 14), the level test down to 1e-2 .. 3e-3
by its level; pooled over every node the level test rejects none of the shares (its 5e5 draws spread over ~7e4 degrees of
freedom), so its verdict on power is the level's.
"""
import math
import os

import numpy as np
import pytest
from scipy import stats

import grad_reference as gr
from conftest import GOLDEN, dense_pauli_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAMES = [r[0] for r in gr.SECTORS]
SUBSET = ["H2", "H2_6-31G", "syn10_3_2", "H2O_6-31G", "syn32_8_8"]          # P = 2, 4, 5, 13, 16
VARIANTS = {"base": {}, "agg": dict(aggregate=True, amp_hidden=128, phase_hidden=(128,)), "phasesym": dict(phase_sym=True),
            "full": dict(masking="FULL"), "none": dict(masking="NONE"), "deep2": dict(amp_layers=2)}
CASES = [(n, "base") for n in NAMES] + [(n, v) for v in VARIANTS if v != "base" for n in SUBSET]
ENUM_MAX = 200_000          # whole space as the key set up to this size
TOP = 50_000                # largest random key set
PV = 1e-4                   # chi-square p-value threshold (test_distribution_matches_psi_squared)
U32 = 2.0 ** -24


def _threads():
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))


def _P(name):
    return gr.sector(name)[1] // 2


def _net(name, variant="base", seed=None, **kw):
    return gr.sector_net(name, seed=_P(name) if seed is None else seed, **VARIANTS[variant], **kw)


def _kdev(keys):
    return torch.as_tensor(np.asarray(keys).astype(np.int64), device="cuda")


def _states(hil, keys):
    return hil.idx2state(torch.as_tensor(np.asarray(keys).astype(np.int64)))


def _whole(hil, seed=5):
    return np.random.RandomState(seed).permutation(hil.restricted2full_idx(np.arange(hil.size)).astype(np.uint64))


def _keyset(hil, M, seed=5):
    return _whole(hil, seed)[:M] if hil.size <= ENUM_MAX else gr.random_keys(hil, M, seed)


def _physical(hil, k):
    """Every key has the sector's electron counts and no bit at or above qubit N (hil.is_physical reads the low N bits)."""
    return bool(hil.is_physical(k).all() and np.all((np.asarray(k, np.uint64) >> np.uint64(hil.N)) == 0))


def _unphysical(hil, M, seed):
    rs = np.random.RandomState(seed)
    cand = np.unique(rs.randint(0, 1 << hil.N, size=8 * M + 64, dtype=np.int64).astype(np.uint64))
    cand = cand[~hil.is_physical(cand)]
    return rs.permutation(cand)[:M]


# ----------------------------------------------------------------------------------------------------- Hamiltonians
_HAM = {}


def _packed(mol):
    """packing_terms.npz's terms of ``mol`` packed as test_packing.py packs them."""
    if mol not in _HAM:
        from naqs_amd import packing, system
        z = np.load(os.path.join(GOLDEN, "packing_terms.npz"))
        terms = {tuple((q, "IXYZ"[o]) for q, o in enumerate(row) if o): c
                 for row, c in zip(z[f"{mol}:ops"].tolist(), z[f"{mol}:coeff"].tolist())}
        m = object.__new__(system.Molecule)
        m.n_electrons, m.multiplicity = (int(v) for v in z[f"{mol}:electrons"])
        n_qubits = packing.n_qubits_of_terms(terms)
        _HAM[mol] = (packing.pack_qubit_hamiltonian(terms, n_qubits, m.get_n_alpha_electrons(), m.get_n_beta_electrons()), terms)
    return _HAM[mol]


def _synthetic_32(keys, seed=17, filtered=True):
    """A 32-qubit Hamiltonian built like test_64bit_keys': flip masks from xors of the keys (and the diagonal)."""
    from naqs_amd import packing
    rs = np.random.RandomState(seed)
    pairs = rs.randint(0, len(keys), size=(300, 2))
    xys = np.unique(np.r_[np.uint64(0), keys[pairs[:, 0]] ^ keys[pairs[:, 1]]])
    xy = np.repeat(xys, rs.randint(1, 6, size=len(xys)))
    yz = rs.randint(0, 1 << 32, size=len(xy), dtype=np.int64).astype(np.uint64)
    cf = rs.normal(size=len(xy))
    perm = rs.permutation(len(xy))
    n = 8 if filtered else -1
    return packing.PackedHamiltonian(32, n, n, xy[perm], yz[perm], cf[perm])


def _row_ham(name, keys):
    """A Hamiltonian on sector ``name``: the molecule's, a random real-symmetric Pauli sum (P = 3, 5), or the 32-qubit one."""
    from naqs_amd import packing
    _, N, na, nb, mol = gr.sector(name)
    if mol is not None:
        return _packed(mol)[0]
    if N == 32:
        return _synthetic_32(np.asarray(keys, np.uint64))
    terms, _, _ = dense_pauli_case(N, 80, 5 + N)
    return packing.pack_qubit_hamiltonian(terms, N, na, nb)


# ---------------------------------------------------------------------------------------------------------- forward
def _kind(variant):
    return {"agg": "agg", "phasesym": "h"}.get(variant, "ws")


def _expect(variant, M, save, cu, ha):
    import test_forward_f64_gpu as tf
    if variant == "deep2":
        import test_amp_depth_gpu as td
        return td._expect(True, M, 2, ha, save=save)
    return tf._expect(_kind(variant), M, save, {}, ha, cu)


def _compare(got, want, P, phase_scale):
    """test_forward_f64_gpu._compare, with the phase bound taken from the largest |phase| of the whole key set (``phase_scale``)
    rather than of the m rows at hand: a default-initialised network's phases are small, and one row's can be far smaller
    than the phase MLP's activations it is rounded from."""
    import test_forward_f64_gpu as tf
    bad, e0, e1, r = tf._compare(got, want, P)
    r1 = e1 / (tf.PHASE_REL * max(tf.PHASE_FLOOR, phase_scale))
    bad = [b for b in bad if not b.startswith("phase")] + ([f"phase {e1:.2e} ({r1:.2f} x bound)"] if not r1 <= 1 else [])
    fin = np.isfinite(want[:, 0]) & np.isfinite(np.asarray(got, np.float64)[:, 0])
    r0 = (np.abs(np.asarray(got, np.float64)[fin, 0] - want[fin, 0]) / tf._bound_log(want[fin, 0], P)).max(initial=0.0)
    return bad, e0, e1, max(r0, r1)


def test_every_sector_gets_a_fused_network():
    """Every row, in every variant, runs on the HIP kernels: the library refuses none of P = 2..16."""
    for name, variant in CASES:
        hil, wf = _net(name, variant)
        assert wf.fused() is not None, (name, variant)


@pytest.mark.parametrize("name,variant", CASES)
def test_forward_against_float64(name, variant):
    import test_forward_f64_gpu as tf
    _threads()
    cu = tf._cus()
    hil, wf = _net(name, variant)
    fused = wf.fused()
    assert fused is not None
    P = hil.N // 2
    L = 2 if variant == "deep2" else 1
    ha = wf.model.amp_layers[0].linears()[0].out_features
    top = min(hil.size, TOP)
    phys = _keyset(hil, top)
    keys = phys
    if VARIANTS[variant].get("masking", "PARTIAL") == "PARTIAL":
        keys = np.random.RandomState(6).permutation(np.concatenate([phys, _unphysical(hil, max(1, top // 4), 7)]))
    sizes = sorted(set(tf._sizes(tf.WS_RB_CAP, len(keys), cu) + [len(keys)]))
    _, wf64 = gr.f64_copy(wf)
    _, wf32 = gr.f64_copy(wf, dtype=torch.float32)
    st = _states(hil, keys)
    ref64, ref32 = gr.log_psi_f64(wf64, st), gr.log_psi_f64(wf32, st)
    assert not np.isnan(ref64).any()
    scale = np.abs(ref64[:, 1]).max()
    fails, worst = [], 0.0
    for m in sizes:
        ks, want, want32 = gr.sorted_rows(keys, m, ref64, ref32)
        k_d = _kdev(ks)
        lp = fused.log_psi(k_d).clone()
        name_k = fused.last_kernel()
        bad, e0, e1, r = _compare(lp.cpu().numpy(), want, P * L, scale)
        _, c0, c1, _ = _compare(want32, want, P * L, scale)
        worst = max(worst, r)
        if name_k != _expect(variant, m, 0, cu, ha):
            bad.append(f"ran {name_k!r}, expected {_expect(variant, m, 0, cu, ha)!r}")
        lpt, _ = fused.forward_saved(k_d)
        if not torch.equal(lpt, lp):
            bad.append("forward_saved differs from naqs_net_logpsi")
        if fused.last_kernel() != _expect(variant, m, 1, cu, ha):
            bad.append(f"training forward ran {fused.last_kernel()!r}")
        print(f"[forward {name} P={P} {variant}] M={m:6d} {name_k}  |HIP - f64| log {e0:.2e} phase {e1:.2e} ({r:.2f} x bound)  "
              f"|torch f32 CPU - f64| log {c0:.2e} phase {c1:.2e}  -inf rows {int((~np.isfinite(want[:, 0])).sum())}")
        fails += [(m, b) for b in bad]
    if variant == "base":
        # naqs_logpsi_eloc: the same log psi and E_loc as the separate calls (physical keys)
        from naqs_amd import hamiltonian
        ks = np.sort(phys[:10000])
        ham = hamiltonian.DevicePauliHamiltonian(_row_ham(name, ks), device="cuda:0")
        k_d = _kdev(ks)
        lp = fused.log_psi(k_d).clone()
        lp2, e2 = fused.log_psi_and_local_energy(ham, k_d)
        e_ref = ham.local_energy(k_d, lp2, kind="log_psi")
        torch.cuda.synchronize()
        ok = torch.equal(lp2, lp) and torch.equal(e2, e_ref) and bool(torch.isfinite(e2).all())
        print(f"[forward+E_loc {name}] M={len(ks)} {fused.last_kernel()}  {'same bits' if ok else 'DIFFERENT'} as the separate calls")
        if not ok:
            fails.append(("logpsi_eloc", len(ks)))
    print(f"[forward {name} P={P} {variant}] worst HIP error {worst:.2f} x bound")
    assert not fails, fails


# --------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("name", NAMES)
def test_backward_against_float64(name):
    _check_backward(name, *_net(name))


def _check_backward(name, hil, wf):
    from test_backward_gpu import BOUND, TAU, W0_FUSE, _dev, _grads, _rel_err, _sums, _zero_grad, _c2
    _threads()
    fused = wf.fused()
    assert fused is not None and fused.train_mode == "hip"
    sizes = sorted({1, min(hil.size, 17), min(hil.size, 3000)} | ({W0_FUSE + 1} if hil.size > W0_FUSE else set()))
    keys = _keyset(hil, max(sizes), 9)
    _, wf64 = gr.f64_copy(wf)
    _, wf32 = gr.f64_copy(wf, dtype=torch.float32)
    rs = np.random.RandomState(11)
    fails, worst = [], 0.0
    for m in sizes:
        ks = np.sort(keys[:m])
        st = _states(hil, ks)
        lp, margin = gr.log_psi_and_kink_margin(wf64, st)
        e = rs.normal(-1.0 * (hil.N // 2), 0.5, m) + 1j * rs.normal(0.0, 1e-3, m)
        w = rs.uniform(0.5, 1.5, m)
        near = margin < TAU
        w[near] = 0.0
        w /= max(w.sum(), 1e-300)
        e_d, w_d, sums_d = _dev(_c2(e)), _dev(w), _dev(_sums(e, w))
        k_d = _kdev(ks)
        _zero_grad(wf)
        fused._grad_flat = None
        _, saved = fused.forward_saved(k_d)
        g1, ev1 = fused.backward_from_local_energy(saved, e_d, w_d, sums_d)
        got1 = _grads(wf)
        _zero_grad(wf)
        fused._grad_flat = None
        _, saved = fused.forward_saved(k_d)
        g2 = fused.vmc_loss_grad(e_d, w_d, sums_d)
        fused.backward_saved(saved, g2)
        got2 = _grads(wf)
        torch.cuda.synchronize()
        # the reference differentiates with the g the loss-gradient kernel handed the backward (held bit for bit to its
        # float32 formula by test_loss_grad_kernel_matches_its_formula): with E_loc uncorrelated with the network,
        # sum_i g_i d log psi_i / d theta cancels to far below its terms, and the float32 rounding of E before E - <E>
        # would dominate the comparison
        g_k = g1.double().cpu().numpy()
        assert np.max(np.abs(g_k - gr.loss_grad_f64(e, w))) <= 1e-5 * np.abs(g_k).max() + 1e-12
        want = gr.grad_f64(wf64, None, g_k, lp=lp)
        want32 = gr.grad_f64(wf32, st, g_k.astype(np.float32))
        same = torch.equal(g1, g2) and all(np.array_equal(got1[n], got2[n]) for n in got1)
        errs = {n: _rel_err(got1[n], want[n]) for n in got1}
        e_hip = max(errs.values())
        e_f32 = max(_rel_err(want32[n], want[n]) for n in got1)
        worst = max(worst, e_hip / BOUND)
        print(f"[backward {name} P={hil.N // 2}] M={m:5d} kink rows {int(near.sum()):3d}  |HIP - f64| {e_hip:.2e} "
              f"({e_hip / BOUND:.2f} x bound)  |torch f32 CPU - f64| {e_f32:.2e}  call forms {'same bits' if same else 'DIFFER'}")
        if not same:
            fails.append((m, "the two call forms differ"))
        fails += [(m, n, r) for n, r in errs.items() if not r <= BOUND]
    print(f"[backward {name}] worst HIP error {worst:.2f} x bound")
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("name", NAMES)
def test_sampler_probs_and_structure(name):
    """probs within 2 (log|psi| bound) + 8 P 2^-24 of exp(2 log|psi|_f64); keys ascending, unique, physical; sum counts <= n."""
    _check_sampler_probs(name, *_net(name))


def _check_sampler_probs(name, hil, wf):
    import test_forward_f64_gpu as tf
    _threads()
    fused = wf.fused()
    n = 10 ** 6
    keys, counts, probs = fused.sample(n, seed=20261016, max_unique=1 << 21)
    k, c, p = keys.cpu().numpy().astype(np.uint64), counts.cpu().numpy(), probs.double().cpu().numpy()
    assert len(k) >= min(hil.size, 4) // 2 and np.all(np.diff(k) > 0) and _physical(hil, k) and (c > 0).all()
    assert c.sum() <= n
    _, wf64 = gr.f64_copy(wf)
    lp = gr.log_amp_f64(wf64, _states(hil, k))
    P = hil.N // 2
    rel = np.abs(p / np.exp(2 * lp) - 1)
    bound = 2 * tf._bound_log(lp, P) + 8 * P * U32
    print(f"[sampler probs {name} P={P}] {len(k)} unique, {c.sum()} kept of {n}  |probs / exp(2 log|psi|_f64) - 1| "
          f"{rel.max():.2e} ({(rel / bound).max():.2f} x bound)")
    assert np.all(rel <= bound), (rel.max(), (rel / bound).max())


# ------------------------------------------------------------------------- every family where the packed offsets round
# A block with 5 or 3 outputs (amplitude spin symmetry, -phase_sym) has a float count that is no multiple of 4, so every
# per-pair offset of the packed copies is rounded: 16-unit blocks at P = 2 and 3, each of the five kinds of handle; the single
# phase MLP of the two SINGLE_PHASE kinds is [16, 16] (test_phase_shapes_gpu.py holds its other widths and depths).
SMALL = {"single": dict(phase_hidden=(16, 16)), "deep": dict(amp_layers=2, phase_hidden=(16, 16)),
         "agg": dict(aggregate=True, phase_hidden=(16,)), "aggdeep": dict(aggregate=True, amp_layers=2, phase_hidden=(16, 16)),
         "comb": dict(combined=True)}
SMALL_KERNEL = {"single": "phase_kernel_h<RB=1, SAVE=0, FMT=2 (f16x2)> + amp_kernel",
                "deep": "phase_kernel_h<RB=1, SAVE=0, FMT=2 (f16x2)> + amp_deep_kernel<1, L=2>", "agg": "agg_finish_kernel",
                "aggdeep": "agg_deep_kernel<1, L=2>", "comb": "comb_head_kernel"}
SMALL_CASES = [(n, f) for n in ("H2", "syn6_2_1") for f in SMALL]


def _small_net(name, family):
    return gr.sector_net(name, seed=_P(name), amp_hidden=16, phase_sym=True, **SMALL[family])


@pytest.mark.parametrize("name,family", SMALL_CASES)
def test_small_blocks_forward_against_float64(name, family):
    """test_forward_against_float64's bounds on the whole space plus unphysical keys; the family's own kernels ran."""
    _threads()
    hil, wf = _small_net(name, family)
    fused = wf.fused()
    assert fused is not None
    m = wf.model
    assert m._n_out_amp == 5 and m._n_out_phase == 3
    P, L = hil.N // 2, len(m.amp_layers[0].linears()) - 1
    keys = np.sort(np.concatenate([_whole(hil), _unphysical(hil, 4, 7)]))
    _, wf64 = gr.f64_copy(wf)
    want = gr.log_psi_f64(wf64, _states(hil, keys))
    assert not np.isnan(want).any()
    k_d = _kdev(keys)
    lp = fused.log_psi(k_d).clone()
    ran = fused.last_kernel()
    bad, e0, e1, r = _compare(lp.cpu().numpy(), want, P * L, np.abs(want[:, 1]).max())
    lpt, _ = fused.forward_saved(k_d)
    print(f"[small forward {name} P={P} {family}] M={len(keys)} {ran}  |HIP - f64| log {e0:.2e} phase {e1:.2e} ({r:.2f} x bound)")
    assert SMALL_KERNEL[family] in ran, ran
    assert torch.equal(lpt, lp), "forward_saved differs from naqs_net_logpsi"
    assert not bad, bad


@pytest.mark.parametrize("name,family", SMALL_CASES)
def test_small_blocks_backward_against_float64(name, family):
    _check_backward(f"{name} {family}", *_small_net(name, family))


@pytest.mark.parametrize("name,family", SMALL_CASES)
def test_small_blocks_sampler_probs(name, family):
    _check_sampler_probs(f"{name} {family}", *_small_net(name, family))


def _chi2(obs, p):
    """test_distribution_matches_psi_squared's binning: bins of >= 5 expected draws, the rest pooled -> (chi2, bins, p-value)."""
    total = obs.sum()
    expect = p / p.sum() * total
    m = expect >= 5
    chi2 = ((obs[m] - expect[m]) ** 2 / expect[m]).sum() + (obs[~m].sum() - expect[~m].sum()) ** 2 / max(expect[~m].sum(), 1e-9)
    return chi2, int(m.sum()), stats.chi2.sf(chi2, m.sum())


SHARES = [1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5]


def _moved(p, src, dst, share):
    """p (a node's conditionals) with ``share`` of child src's mass moved to child dst."""
    q = p.copy()
    q[src] -= share * p[src]
    q[dst] += share * p[src]
    return q


EXACT = [(n, "base") for n in NAMES if math.comb(gr.sector(n)[1] // 2, gr.sector(n)[2])
         * math.comb(gr.sector(n)[1] // 2, gr.sector(n)[3]) <= 2_000_000] + [("H2", "deep2"), ("H2_6-31G", "deep2"),
                                                                           ("syn10_3_2", "deep2")]


@pytest.mark.parametrize("name,variant", EXACT)
def test_sampler_exact_chi2(name, variant):
    """The draws over the whole physical space against exp(2 log|psi|) of the float64 amplitude blocks: 10^9 draws (over 600
    per state at P = 13; fewer draws leave the chi-square blind to a 1 % change of the root's conditionals).  Power check on the host with the same draws: the reference with a
    share of the root's largest child moved to its smallest physical child must be rejected (reported: the smallest share)."""
    _threads()
    hil, wf = _net(name, variant)
    fused = wf.fused()
    n = 10 ** 9
    keys, counts, _ = fused.sample(n, seed=20240607, max_unique=hil.size + 16)
    if variant == "deep2":
        assert "sample_expand_deep_kernel" in fused.last_kernel()
    k, c = keys.cpu().numpy().astype(np.uint64), counts.cpu().numpy()
    assert np.all(np.diff(k) > 0) and _physical(hil, k) and c.sum() <= n
    all_keys = np.sort(hil._all_keys()).astype(np.uint64)
    pos = np.searchsorted(all_keys, k)
    assert np.array_equal(all_keys[pos], k)
    obs = np.zeros(len(all_keys))
    obs[pos] = c
    _, wf64 = gr.f64_copy(wf)
    st = _states(hil, all_keys)
    p = np.exp(2 * gr.log_amp_f64(wf64, st))
    chi2, bins, pv = _chi2(obs, p)
    # the power check: the root's conditionals with mass moved between two of its children
    p0, phys0 = gr.conditionals_f64(wf64, st[:1], 0)
    p0, phys0 = p0[0], phys0[0]
    order = [j for j in np.argsort(-p0) if phys0[j]]
    src, dst = order[0], order[-1]
    ms = st[:, wf64._q2m.cpu()]
    child0 = ((ms[:, 0] > 0).long() + 2 * (ms[:, 1] > 0).long()).numpy()
    rejected = []
    for s in SHARES:
        ratio = _moved(p0, src, dst, s) / np.where(p0 > 0, p0, 1)
        if _chi2(obs, p * ratio[child0])[2] < PV:
            rejected.append(s)
    print(f"[sampler chi2 {name} P={hil.N // 2} {variant}] n={n:.2e} space {hil.size} unique {len(k)} bins {bins} "
          f"chi2 {chi2:.1f} p-value {pv:.3g}  {fused.last_kernel()}  power: rejects a moved share down to "
          f"{min(rejected) if rejected else 'NONE'}")
    assert pv > PV, (chi2, bins, pv)
    assert SHARES[0] in rejected, "the exact chi-square cannot tell a 1 % change of the root's conditionals"


def _tree_levels(wf64, hil, k, c):
    return gr.tree_levels(wf64, hil, k, c)


def _tree_chi2(levels, root=None):
    """grad_reference.tree_chi2 (FULL masking: no draw is dropped)."""
    return gr.tree_chi2(levels, root=root)[:5]


@pytest.mark.parametrize("name", ["BeH2", "Li2O", "syn32_8_8"])
def test_sampler_level_by_level(name):
    """For spaces too large to enumerate (and BeH2 beside its exact chi-square): FULL masking, each node's children counts
    against Multinomial(count, float64 conditionals), masked children exactly 0.  Verdict: the chi-square pooled over every
    node, and each level's (at 1e-4 / P).  Power check: a share of the root's largest child moved to its smallest physical
    one must be rejected by its level."""
    _threads()
    hil, wf = _net(name, "full")
    fused = wf.fused()
    n = 500_000
    keys, counts, _ = fused.sample(n, seed=4242, max_unique=1 << 21)
    k, c = keys.cpu().numpy().astype(np.uint64), counts.cpu().numpy()
    assert c.sum() == n and np.all(np.diff(k) > 0) and _physical(hil, k)
    _, wf64 = gr.f64_copy(wf)
    P = hil.N // 2
    tree = _tree_levels(wf64, hil, k, c)
    chi2, dof, pv, levels, masked = _tree_chi2(tree)
    p0, phys0 = gr.conditionals_f64(wf64, _states(hil, k[:1]), 0)
    order = [j for j in np.argsort(-p0[0]) if phys0[0][j]]
    rejected = []
    for s in SHARES:
        _, _, pv_s, lv_s, _ = _tree_chi2(tree, root=_moved(p0[0], order[0], order[-1], s))
        if min(lv_s) < PV / P:
            rejected.append((s, pv_s < PV))
    print(f"[sampler levels {name} P={P}] n={n} unique {len(k)}  pooled chi2 {chi2:.1f} dof {dof} p-value {pv:.3g}  "
          f"level p-values {' '.join('%.2g' % v for v in levels)}  masked children drawn {masked}  power: rejects down to "
          f"{min(s for s, _ in rejected) if rejected else 'NONE'} by its level (pooled over all nodes down to "
          f"{min([s for s, b in rejected if b], default='NONE')})")
    assert masked == 0
    assert pv > PV and min(levels) > PV / P, (pv, levels)
    assert rejected and rejected[0][0] == SHARES[0], "the level test cannot tell a 1 % change of the root's conditionals"


FUSIONS = (("2", "1", "1"), ("1", "1", "1"), ("0", "1", "1"), ("2", "0", "1"), ("0", "0", "1"), ("1", "1", "3"), ("1", "1", "2"),
           ("0", "1", "3"), ("2", "1", "2"), ("1", "1", "4"), ("0", "1", "4"))


@pytest.mark.parametrize("name", NAMES)
def test_launch_fusions_change_nothing(name, monkeypatch):
    """test_sampler_gpu.py's launch cuts (head of 5 / 4 / no levels, fused or split levels, 1..4 levels per launch) at every
    P: the same draws bit for bit, and the same overflow outcome at caps around the final size."""
    from naqs_amd.nade import MaxBatchSizeExceededError
    hil, wf = _net(name)
    fused = wf.fused()
    n = 10 ** 6 if hil.size < 10 ** 5 else 30_000

    def draw(head, fuse, multi, cap):
        monkeypatch.setenv("NAQS_SAMPLE_HEAD", head)
        monkeypatch.setenv("NAQS_SAMPLE_FUSED", fuse)
        monkeypatch.setenv("NAQS_SAMPLE_MULTI", multi)
        fused.sample(n, seed=76, max_unique=1 << 20)
        try:
            return fused.sample(n, seed=77, max_unique=cap)
        except MaxBatchSizeExceededError:
            return None

    outs = [draw(*f, 1 << 20) for f in FUSIONS]
    M = len(outs[0][0])
    assert M >= min(hil.size, 4) // 2
    for f, o in zip(FUSIONS[1:], outs[1:]):
        assert all(torch.equal(x, y) for x, y in zip(outs[0], o)), (name, f)
    verdicts = []
    for cap in sorted({max(1, M - 1), M, M + M // 8, 2 * M}):
        res = [draw("1", "1", multi, cap) for multi in ("1", "2", "4")]
        verdicts.append((cap, res[0] is not None))
        assert (res[0] is None) == (res[1] is None) == (res[2] is None), cap
        if res[0] is not None:
            assert all(torch.equal(x, y) for r in res[1:] for x, y in zip(res[0], r))
        if cap == M - 1:
            assert res[0] is None
    print(f"[sampler launches {name} P={hil.N // 2}] n={n} M={M}  caps (fits): {verdicts}")
    for k in ("NAQS_SAMPLE_HEAD", "NAQS_SAMPLE_FUSED", "NAQS_SAMPLE_MULTI"):
        monkeypatch.delenv(k)


# ---------------------------------------------------------------------------------------- the library training loop
LOOP = ["H2", "H2_6-31G", "syn10_3_2"]          # P = 2, 4, 5 (the first P whose update launch packs head pairs)


def _opt(name, tmp, net_kw=None, **kw):
    """``net_kw``: passed to the network (``qubit_ordering``: test_qubit_ordering_gpu.py); ``kw``: to the optimiser."""
    from naqs_amd.optimizer import PartialSamplingOptimizer
    from test_optimizer import ADAM
    hil, wf = _net(name, **(net_kw or {}))
    _, N, na, nb, _ = gr.sector(name)
    args = dict(n_samples=100000, n_samples_max=1e12, n_unq_samples_min=2, n_unq_samples_max=1e5, log_exact_energy=False,
                wavefunction=wf, qubit_hamiltonian=_row_ham(name, None), pre_compute_H=False, n_electrons=na + nb,
                n_alpha_electrons=na, n_beta_electrons=nb, normalise_psi=True, grad_clip_factor=None,
                optimizer=torch.optim.Adam, optimizer_args=[dict(a) for a in ADAM], save_loc=str(tmp),
                pauli_hamiltonian_dtype=np.float64, seed=5)
    args.update(kw)
    return hil, wf, PartialSamplingOptimizer(**args)


@pytest.mark.parametrize("name", LOOP)
def test_library_loop_equals_step_by_step(name, tmp_path, monkeypatch):
    """naqs_vmc_run over 20 steps against one naqs_vmc_step per step: energies, sample counts and parameters bit for bit."""
    _loop_equals_step_by_step(name, tmp_path, monkeypatch, 20)


def _loop_equals_step_by_step(name, tmp_path, monkeypatch, steps, **net_kw):
    from naqs_amd.optimizer import LogKey
    runs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("NAQS_TRAIN_RUN", mode)
        hil, wf, opt = _opt(name, tmp_path / mode, net_kw=net_kw)
        assert opt._can_onecall() and opt._can_run_in_library() == (mode == "1")
        opt.run(n_epochs=steps, save_freq=None, save_final=False, output_freq=10 ** 9)
        runs[mode] = (np.array(opt.log[LogKey.E_LOC]), np.array(opt.log[LogKey.N_UNIQUE_SAMP]), wf.flatten_parameters().clone())
    a, b = runs["1"], runs["0"]
    print(f"[library loop {name} {net_kw or ''}] {steps} steps, <E> {a[0][0, 1]:.6f} -> {a[0][-1, 1]:.6f}")
    assert len(a[0]) == steps and np.isfinite(a[0]).all()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("overlap", ["2", "1", "0"])
@pytest.mark.parametrize("name", LOOP)
def test_forward_after_library_training_steps(name, overlap, tmp_path, monkeypatch):
    """test_forward_f64_gpu.py's trained-network check at P <= 5 (the re-pack of the first pairs goes ahead of a head-less
    sampler there): after 50 library steps with no refresh, the forward of the whole space against the float64 copy of the
    current parameters in every NAQS_PACK_OVERLAP mode."""
    _forward_after_training(name, overlap, tmp_path, monkeypatch, 50)


def _forward_after_training(name, overlap, tmp_path, monkeypatch, steps, **net_kw):
    _threads()
    monkeypatch.setenv("NAQS_PACK_OVERLAP", overlap)
    hil, wf, opt = _opt(name, tmp_path, net_kw=net_kw)
    assert opt._can_onecall()
    p0 = wf.flatten_parameters().clone()
    opt.run(n_epochs=steps, save_freq=None, save_final=False, output_freq=10 ** 9)
    torch.cuda.synchronize()
    fused = wf._fused
    assert fused is not None and fused is not False
    assert not torch.equal(wf.flatten_parameters(), p0)
    _, wf64 = gr.f64_copy(wf)
    keys = np.sort(hil._all_keys()).astype(np.uint64)
    want = gr.log_psi_f64(wf64, _states(hil, keys))
    lp = fused.log_psi(_kdev(keys))
    bad, e0, e1, r = _compare(lp.cpu().numpy(), want, hil.N // 2, np.abs(want[:, 1]).max())
    print(f"[trained {name} {net_kw or ''} NAQS_PACK_OVERLAP={overlap}] M={len(keys)} {fused.last_kernel()}  |HIP - f64| log {e0:.2e} "
          f"phase {e1:.2e} ({r:.2f} x bound)")
    assert not bad, bad


def _sector_matrix(name):
    """The dense Hamiltonian of ``name``'s sector from its Pauli terms (qubit q <-> bit q, |1> = occupied), and its keys."""
    from naqs_amd.hilbert import Hilbert
    _, N, na, nb, mol = gr.sector(name)
    terms = _packed(mol)[1]
    sig = {"I": np.eye(2, dtype=complex), "X": np.array([[0, 1], [1, 0]], complex),
           "Y": np.array([[0, -1j], [1j, 0]], complex), "Z": np.array([[1, 0], [0, -1]], complex)}
    H = np.zeros((1 << N, 1 << N), complex)
    for ops, c in terms.items():
        d = dict(ops)
        m = np.eye(1, dtype=complex)
        for q in range(N):
            m = np.kron(sig[d.get(q, "I")], m)
        H += c * m
    keys = np.sort(Hilbert.get(N, na, nb)._all_keys())
    return H[np.ix_(keys, keys)], keys


@pytest.mark.parametrize("name,steps", [("H2", 500), ("H2_6-31G", 1000)])
def test_library_loop_reaches_the_ground_state(name, steps, tmp_path):
    """H2 (4 states) and H2_6-31G (16): the library loop, with the reference's Adam settings, trains to within 0.1 mHa of the
    lowest eigenvalue of the sector's dense Hamiltonian (energy of the network's normalised psi over the whole sector).  H2
    gets there in 400 steps, H2_6-31G in 700 (0.48 mHa after 500).  With eps = 1e-15 every Adam step moves each parameter by
    about lr: lr = 1e-3 bounds how fast the last fraction of a mHa goes, and larger rates (2e-3 .. 5e-3) overshoot."""
    Hs, keys = _sector_matrix(name)
    assert np.max(np.abs(Hs - Hs.conj().T)) < 1e-12
    e0 = np.linalg.eigvalsh(Hs)[0]
    hil, wf, opt = _opt(name, tmp_path)
    gap = []
    for _ in range(steps // 100):
        opt.run(n_epochs=100, save_freq=None, save_final=False, output_freq=10 ** 9)
        lp = wf.fused().log_psi(_kdev(keys)).double().cpu().numpy()
        psi = np.exp(lp[:, 0] + 1j * lp[:, 1])
        psi /= np.linalg.norm(psi)
        gap.append(float((psi.conj() @ Hs @ psi).real - e0))
        if gap[-1] < 1e-4:
            break
    print(f"[ground state {name}] E0 {e0:.8f}  <H> - E0 after each 100 steps: {['%.2e' % g for g in gap]}")
    assert gap[-1] < 1e-4, gap


# -------------------------------------------------------------------------------------------------------------- E_loc
_MOLS = sorted({k.split(":")[0] for k in np.load(os.path.join(GOLDEN, "packing_terms.npz")).files})


def _eloc(ham, keys, psi):
    from naqs_amd import hamiltonian
    k = hamiltonian.keys_to_device(np.asarray(keys, np.uint64), ham.device)
    e = ham.local_energy(k, torch.as_tensor(np.stack([psi.real, psi.imag], -1), dtype=torch.float64, device=ham.device), kind="psi")
    torch.cuda.synchronize()
    e = e.cpu().numpy()
    return e[:, 0] + 1j * e[:, 1]


def _rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))) if len(a) else 0.0


@pytest.mark.parametrize("mol", _MOLS)
def test_eloc_of_every_shipped_hamiltonian(mol, monkeypatch):
    """Every molecule of packing_terms.npz: E_loc at up to 2 000 clustered keys (the whole sector where smaller) against the
    oracle; most rows couple; the chunk length the handle derives from the sector (64 where it has more than 2^20 states —
    H2O_6-31G, Li2O —, 8 elsewhere) gives the bits of a handle forced to that length, and both lengths match the oracle."""
    from naqs_amd import hamiltonian
    from oracle import oracle
    from test_eloc_gpu import all_keys, clustered_keys, synth_logpsi
    ham_p, _ = _packed(mol)
    N, na, nb = ham_p.n_qubits, ham_p.n_alpha, ham_p.n_beta
    size = math.comb(N // 2, na) * math.comb(N // 2, nb)
    h = dict(n_qubits=N, n_alpha=na, n_beta=nb, xy=ham_p.xy)
    keys = all_keys(N, na, nb) if size <= 2000 else clustered_keys(h, 2000, 21)
    assert len(keys) >= min(size, 250), len(keys)
    lp = synth_logpsi(len(keys), 12)
    psi = np.exp(lp[:, 0] + 1j * lp[:, 1])
    monkeypatch.delenv("NAQS_CHUNK_TERMS", raising=False)
    ham = hamiltonian.DevicePauliHamiltonian(ham_p, device="cuda:0")
    e = _eloc(ham, keys, psi)
    kern = ham.last_kernel()
    want = oracle.eloc_matrix_free(ham_p.xy, ham_p.yz, ham_p.coeff, keys, psi)
    n_conn = np.count_nonzero(np.abs(want - want.real.mean()) > 0)
    chunk = 64 if math.log2(size) > 20 else 8
    forced = {}
    for c in (8, 64):
        monkeypatch.setenv("NAQS_CHUNK_TERMS", str(c))
        forced[c] = _eloc(hamiltonian.DevicePauliHamiltonian(ham_p, device="cuda:0"), keys, psi)
    monkeypatch.delenv("NAQS_CHUNK_TERMS")
    errs = {c: _rel(forced[c], want) for c in forced}
    print(f"[E_loc {mol}] {N} qubits ({na}, {nb}) K={ham_p.K} space {size} M={len(keys)} coupled {n_conn}  {kern}  "
          f"|HIP - oracle| {_rel(e, want):.1e}  chunk {chunk}: same bits {np.array_equal(e, forced[chunk])}  "
          f"forced 8 / 64: {errs[8]:.1e} / {errs[64]:.1e}")
    assert _rel(e, want) < 1e-10
    assert n_conn > len(keys) // 2
    assert np.array_equal(e, forced[chunk]), "the default handle does not use the chunk length its sector selects"
    assert errs[8] < 1e-10 and errs[64] < 1e-10


@pytest.mark.parametrize("filtered", [True, False])
def test_eloc_32bit_keys_with_bit31(filtered):
    """32 qubits, 8 + 8 electrons: the 32-bit key path (key_bits == 32) with keys that have bit 31 set, against the oracle,
    with the sector filter and without, and with the Bloom filter forced on."""
    from naqs_amd import hamiltonian
    from oracle import oracle
    from test_eloc_gpu import random_physical_keys, synth_logpsi
    keys = random_physical_keys(32, 8, 8, 3000, 31)
    hi = (keys >> np.uint64(31)) & np.uint64(1)
    assert hi.sum() > 1000 and (hi == 0).sum() > 1000
    ham_p = _synthetic_32(keys, filtered=filtered)
    ham = hamiltonian.DevicePauliHamiltonian(ham_p, device="cuda:0")
    assert ham.key_bits == 32
    lp = synth_logpsi(len(keys), 3)
    psi = np.exp(lp[:, 0] + 1j * lp[:, 1])
    want = oracle.eloc_matrix_free(ham_p.xy, ham_p.yz, ham_p.coeff, keys, psi)
    assert np.count_nonzero(np.abs(want) > 0) > 100
    e = _eloc(ham, keys, psi)
    kern = ham.last_kernel()
    assert _rel(e, want) < 1e-10, _rel(e, want)
    for extra in ({"NAQS_BLOOM": "1", "NAQS_BLOCK": "1024"}, {"NAQS_ELOC_V": "1", "NAQS_BLOOM": "1", "NAQS_BLOCK": "1024"}):
        os.environ.update(extra)
        try:
            e2 = _eloc(ham, keys, psi)
            kern2 = ham.last_kernel()
        finally:
            for k in extra:
                del os.environ[k]
        print(f"[E_loc 32-bit keys filtered={filtered}] {kern} / {extra}: {kern2}  |HIP - oracle| {_rel(e2, want):.1e}")
        assert _rel(e2, want) < 1e-10, (extra, _rel(e2, want))
