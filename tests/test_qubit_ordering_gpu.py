"""The network, sampler and training-step kernels on the MI355X at qubit orderings other than the default -1.

naqs_net_config_t::qubit2model becomes NetDims::qa[] / qb[] (net_layout, naqs_logpsi.hip), which every kernel uses to pull the
model-order occupations out of a key (amp_item, the phase kernels' input stage, amp2_kernel / agg_finish_kernel, the combined
and deep kernels, the backward kernels, phase_inputs_kernel) and the sampler uses to put a key back together (three sites of
naqs_sample.hip).  Every other GPU test builds its network at -1, where model pair n sits on key bits N-2-2n / N-1-2n and the
sampler's (prefix, outcome) order is ascending key order.  Here: ordering +1 (model pair n = orbital pair n) and a seeded
spin-preserving pair permutation pi (grad_reference.pair_ordering), for every kind of handle.  CPU counterpart (the torch
formulation, and the helpers): test_qubit_ordering.py.

(a) Relabelling invariance, bit for bit.  Handle A at -1 and handle B at ordering O with A's state_dict; keys_B[i] =
    relabel_keys(keys_A[i]) shows B the model-order bits keys_A[i] shows A.  Every kernel reduces a key to (abits, bbits) before
    any arithmetic, rows are independent in the forward and the backward's reductions run in fixed row order: torch.equal on
    log psi (naqs_net_logpsi, the training forward, naqs_logpsi_eloc), naqs_net_logamp, the flat gradient of forward_saved +
    backward_saved and naqs_net_amp_backward — with keys_A ascending (at -1: rows sharing model prefixes are neighbours) and in
    a random row order.  No form needed a tolerance.  naqs_net_phase_inputs against numpy from q2m, and the blas training
    mode / log_psi_train (FusedLogPsi._phase_shifts reads the same bits).
(b) Float64 anchors at ordering O itself: handle B against gr.f64_copy(B) with test_forward_f64_gpu's bounds (through
    test_pairs_gpu._compare: the same constants, the phase scale taken from the case's whole key set, and P x L pairs for L
    amplitude layers, as that module does for default-initialised and deep networks) and test_backward_gpu's BOUND, kink rows
    zeroed at TAU (at most 10 % of the rows).
(c) The sampler: the same seed draws keys_B == relabel_keys(keys_A) element by element with equal counts, probs and weights,
    under the launch cuts that reach each of the three key-assembly sites; at O the table is strictly increasing in
    model_index (not in key), physical, and its probs are exp(2 log|psi|) of float64; an exact chi-square at +1; the same
    overflow verdicts.
(d) The step: naqs_vmc_run against naqs_vmc_step at +1, the trained handle against float64, the reference's own vectors at
    +1 (nade_LiH_qo1.npz, through test_variants_gpu.py / test_backward_gpu.py) and one CLI run with -qo 1.

Measured on an MI355X (the module: 11 s), worst HIP error in units of the bound, forward / backward; +1 and pi give the same
figures to the digit (the same model-order bits reach the same arithmetic) and every case was bit for bit equal to -1:
published shape 0.25 / 0.04 (LiH), 0.26 / 0.08 (LiF), 0.34 / 0.03 (32 qubits); phase_kernel_h 0.25 / 0.03, with -phase_sym
0.25 / 0.03; aggregate 0.29 / 0.04, with -phase_sym 0.28 / 0.03; combined 0.25 / 0.04; deep amplitude 0.14 / 0.17; deep
aggregate 0.11 / 0.04; NAQS_AMP_MODE 0 / 1 / 2 0.23 / 0.25 / 0.25 (backward 0.03); FULL masking with unphysical keys 0.24 / 0.03;
the trained handles 0.30 (LiH), 0.28 (LiF); the sampler's probs 0.04 .. 0.10; chi-square p-value 0.36.  At -1 the same
bounds see <= 0.47 (forward, test_forward_f64_gpu.py), 0.18 (backward) and 0.10 (probs, test_pairs_gpu.py); float32 PyTorch
on the CPU errs by about as much on the same rows (printed beside each case).
"""
import numpy as np
import pytest

import grad_reference as gr
from test_qubit_ordering import FORMS, ORDERINGS, PV, chi2_pvalue, ordering

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# family -> (form of test_qubit_ordering.FORMS, sectors, environment)
FAMILIES = {
    "ws": ("ws", ["LiH", "LiF", "syn32_8_8"], {}),
    "h": ("h", ["H2", "syn10_3_2", "LiF"], {}),
    "h_phasesym": ("h_phasesym", ["H2", "syn10_3_2", "LiF"], {}),
    "agg": ("agg", ["LiH", "LiF"], {}),
    "agg_phasesym": ("agg_phasesym", ["LiH", "LiF"], {}),
    "comb": ("comb", ["LiH", "O2"], {}),
    "deep": ("deep", ["LiH", "syn32_8_8"], {}),
    "aggdeep": ("aggdeep", ["LiH"], {}),
    "amp0": ("ws", ["LiF"], {"NAQS_AMP_MODE": "0"}),
    "amp1": ("ws", ["LiF"], {"NAQS_AMP_MODE": "1"}),
    "amp2": ("ws", ["LiF"], {"NAQS_AMP_MODE": "2"}),
    "full": ("full", ["LiF"], {}),
}
# (H2 has two orbital pairs: no permutation besides +1 and -1, so no "pi" case)
CASES = [(f, n, t) for f, (_, names, _) in FAMILIES.items() for n in names for t in ORDERINGS if not (n == "H2" and t == "pi")]
RAN = {"h": "phase_kernel_h<", "h_phasesym": "phase_kernel_h<", "agg": "amp2_kernel + agg_finish_kernel",
       "agg_phasesym": "amp2_kernel + agg_finish_kernel", "comb": "comb_head_kernel", "deep": "amp_deep_kernel<",
       "aggdeep": "agg_deep_kernel<"}
ENUM_MAX = 2000         # the whole space as the key set up to this size


def _kdev(keys):
    return torch.as_tensor(np.asarray(keys).astype(np.int64), device="cuda")


def _states(hil, keys):
    return hil.idx2state(torch.as_tensor(np.asarray(keys).astype(np.int64)))


def _pair(name, form, O, seed=3):
    """(hilbert, network A at -1, network B at ordering O with A's state_dict, q2m of A, q2m of B)."""
    hil, wfA = gr.sector_net(name, seed=seed, **FORMS[form])
    _, wfB = gr.sector_net(name, seed=seed + 1, qubit_ordering=O, **FORMS[form])
    wfB.model.load_state_dict(wfA.model.state_dict())
    qA, qB = gr.q2m_of(-1, hil.N), gr.q2m_of(O, hil.N)
    assert [int(q) for q in wfA.qubit2model_permutation] == qA and [int(q) for q in wfB.qubit2model_permutation] == qB
    assert qA != qB
    return hil, wfA, wfB, qA, qB


def _flat_grad(wf):
    return torch.cat([p.grad.reshape(-1) for p in wf.param_list()]).clone()


def _run_all(fused, wf, k_d, g_d, ham, back=None):
    """Every entry point of (a) on one handle -> dict of device tensors (clones) + the forward's kernel name.  ``back``: the
    rows the backward runs on (the physical ones of a table with unphysical keys: a row of probability zero has no
    gradient), all rows when None."""
    from naqs_amd import _lib
    from naqs_amd.hamiltonian import _stream_ptr
    import test_backward_gpu as tb
    M = k_d.shape[0]
    out = {"log_psi": fused.log_psi(k_d).clone()}
    ran = fused.last_kernel()
    out["forward_saved"] = fused.forward_saved(k_d)[0].clone()
    k_b, g_b = (k_d, g_d) if back is None else (k_d[back].contiguous(), g_d[back].contiguous())
    out["grad"] = torch.zeros(fused.n_params, dtype=torch.float32, device="cuda")
    out["amp_backward"] = torch.zeros(fused.n_amp_params, dtype=torch.float32, device="cuda")
    if k_b.shape[0]:
        tb._zero_grad(wf)
        fused._grad_flat = None
        _, saved = fused.forward_saved(k_b)
        fused.backward_saved(saved, g_b)
        out["grad"] = _flat_grad(wf)
        ga = g_b[:, 0].contiguous()
        flat = torch.full((fused.n_amp_params,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(fused._lib.naqs_net_amp_backward(fused._h, k_b.shape[0], k_b.data_ptr(), ga.data_ptr(), flat.data_ptr(),
                                                    _stream_ptr(fused.device)), "naqs_net_amp_backward")
        out["amp_backward"] = flat
    la = torch.full((M,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(fused._lib.naqs_net_logamp(fused._h, M, k_d.data_ptr(), la.data_ptr(), _stream_ptr(fused.device)), "naqs_net_logamp")
    out["logamp"] = la
    if ham is not None:
        out["logpsi_eloc"] = fused.log_psi_and_local_energy(ham, k_d)[0].clone()
    torch.cuda.synchronize()
    return out, ran


# -------------------------------------------------------------------------------------- (a) + (b): forward and backward
@pytest.mark.parametrize("family,name,tag", CASES)
def test_relabelling_invariance_and_float64_anchors(family, name, tag, monkeypatch):
    import test_backward_gpu as tb
    import test_forward_f64_gpu as tf
    import test_pairs_gpu as tp
    from naqs_amd import hamiltonian
    tp._threads()
    form, _, env = FAMILIES[family]
    tf._set_env(monkeypatch, env)
    cu = tf._cus()
    P = gr.sector(name)[1] // 2
    O = ordering(tag, P)
    hil, wfA, wfB, qA, qB = _pair(name, form, O)
    fA, fB = wfA.fused(), wfB.fused()
    assert fA is not None and fB is not None and fA.train_mode == "hip"
    L = len(wfA.model.amp_layers[0].linears()) - 1
    ha = wfA.model.amp_layers[0].linears()[0].out_features

    # rows: the whole space where small, otherwise 1 / 17 / 1000 random keys (and the published shape's SPLIT and RB edges)
    if hil.size <= ENUM_MAX:
        sizes = [hil.size]
        keysA = tb._whole_space(hil, 5)
    else:
        sizes = [1, 17, 1000] + ([tf._split_limit(cu) + 1, tf.TILE * cu + 1] if (family, name) == ("ws", "LiF") else [])
        keysA = gr.random_keys(hil, max(sizes), 5)
    if family == "full":
        keysA = tf._unphysical_mix(hil, max(sizes), 5)
    keysB = gr.relabel_keys(keysA, qA, qB)
    assert np.array_equal(hil.is_physical(keysA), hil.is_physical(keysB)) and not np.array_equal(keysA, keysB)
    M = len(keysA)
    assert M == max(sizes)

    # float64 / float32 references of B at ordering O, once, on the whole key set; kink rows get g = 0
    _, B64 = gr.f64_copy(wfB)
    _, B32 = gr.f64_copy(wfB, dtype=torch.float32)
    stB = _states(hil, keysB)
    ref64, ref32 = gr.log_psi_f64(B64, stB), gr.log_psi_f64(B32, stB)
    assert not np.isnan(ref64).any()
    ninf = ~np.isfinite(ref64[:, 0])
    if family == "full":
        assert ninf.sum() >= M // 5
    else:
        assert not ninf.any()
    scale = np.abs(ref64[:, 1]).max()
    g = np.random.RandomState(7).normal(size=(M, 2)).astype(np.float32).astype(np.float64) / np.sqrt(M)
    g[ninf] = 0                                     # (a row of probability zero has no gradient: left out of the backward)
    fin = np.flatnonzero(~ninf)
    pos = {m: int((fin < m).sum()) for m in sizes}  # finite rows among the first m
    g_fin = g[fin]
    grad64, margin = tb._segment_grads(B64, stB[fin], g_fin, [pos[m] for m in sizes if pos[m]], tau=tb.TAU)
    g[fin] = g_fin
    n_kink = int((margin < tb.TAU).sum())
    assert n_kink <= 0.1 * M, (n_kink, M)
    grad32, _ = tb._segment_grads(B32, stB[fin], g[fin].astype(np.float32), [pos[m] for m in sizes if pos[m]])

    ham = None
    if family != "full":
        ham = hamiltonian.DevicePauliHamiltonian(tp._row_ham(name, keysA), device="cuda:0")

    fails, worst_f, worst_b = [], 0.0, 0.0
    for m in sizes:
        for order_name, rows in (("ascending", np.argsort(keysA[:m], kind="stable")), ("random", np.arange(m))):
            kA, kB, g_d = _kdev(keysA[:m][rows]), _kdev(keysB[:m][rows]), tb._dev(g[:m][rows], torch.float32)
            back = None if family != "full" else torch.as_tensor(np.flatnonzero(~ninf[:m][rows]), device="cuda")
            outA, ranA = _run_all(fA, wfA, kA, g_d, ham, back)
            outB, ranB = _run_all(fB, wfB, kB, g_d, ham, back)
            where = (m, order_name)
            # (a) bit for bit
            for what in outA:
                if not torch.equal(outA[what], outB[what]):
                    d = np.abs(outA[what].double().cpu().numpy() - outB[what].double().cpu().numpy())
                    fails.append((where, f"{what} differs between -1 and {tag}: max |d| {np.nanmax(d[np.isfinite(d)], initial=0.0):.2e} ({ranB})"))
            if not torch.equal(outB["forward_saved"], outB["log_psi"]) or (ham is not None and not torch.equal(outB["logpsi_eloc"], outB["log_psi"])):
                fails.append((where, "the training forward / naqs_logpsi_eloc differ from naqs_net_logpsi at ordering O"))
            if ranA != ranB:
                fails.append((where, f"ran {ranB!r} at {tag}, {ranA!r} at -1"))
            exp_name = tf._expect("ws", m, 0, env, ha, cu) if form in ("ws", "full") else RAN[family]
            if (ranB != exp_name) if form in ("ws", "full") else (exp_name not in ranB):
                fails.append((where, f"ran {ranB!r}, expected {exp_name!r}"))
            # (b) float64 at ordering O
            bad, e0, e1, r = tp._compare(outB["log_psi"].cpu().numpy(), ref64[:m][rows], P * L, scale)
            _, c0, c1, _ = tp._compare(ref32[:m][rows], ref64[:m][rows], P * L, scale)
            la = outB["logamp"].double().cpu().numpy()
            okr = ~ninf[:m][rows]
            r_la = (np.abs(la[okr] - ref64[:m][rows][okr, 0]) / tf._bound_log(ref64[:m][rows][okr, 0], P * L)).max(initial=0.0)
            if not r_la <= 1 or not np.array_equal(la == -np.inf, ~okr):
                bad.append(f"naqs_net_logamp {r_la:.2f} x bound")
            worst_f = max(worst_f, r, r_la)
            fails += [(where, b) for b in bad]
            e_hip = e_f32 = 0.0
            if pos[m]:
                got, flat, off = {}, outB["grad"].double().cpu().numpy(), 0
                for n_, p in wfB.model.named_parameters():
                    got[n_] = flat[off:off + p.numel()].reshape(tuple(p.shape))
                    off += p.numel()
                errs = {n_: tb._rel_err(got[n_], grad64[pos[m]][n_]) for n_ in got}
                e_hip = max(errs.values())
                e_f32 = max(tb._rel_err(grad32[pos[m]][n_], grad64[pos[m]][n_]) for n_ in got)
                worst_b = max(worst_b, e_hip / tb.BOUND)
                fails += [(where, n_, e) for n_, e in errs.items() if not e <= tb.BOUND]
            print(f"[ordering {family} {name} P={P} {tag}] M={m:5d} {order_name:9s} {ranB}  -1 vs {tag}: "
                  f"{'same bits' if not any(f[0] == where and 'differs' in str(f[1]) for f in fails) else 'DIFFERENT'}  "
                  f"|HIP - f64| log {e0:.2e} phase {e1:.2e} ({r:.2f} x bound; logamp {r_la:.2f})  |torch f32 CPU - f64| log {c0:.2e} "
                  f"phase {c1:.2e}  backward |HIP - f64| {e_hip:.2e} ({e_hip / tb.BOUND:.2f} x bound) |torch f32 CPU - f64| {e_f32:.2e}  "
                  f"kink rows {int((margin[:pos[m]] < tb.TAU).sum())}")
    tf._set_env(monkeypatch, {})
    print(f"[ordering {family} {name} {tag}] worst HIP error: forward {worst_f:.2f} x bound, backward {worst_b:.2f} x bound")
    assert not fails, fails


@pytest.mark.parametrize("tag", ORDERINGS)
@pytest.mark.parametrize("name,form", [("LiH", "h"), ("LiF", "ws"), ("syn32_8_8", "ws")])
def test_phase_inputs_and_blas_training_mode(name, form, tag):
    """naqs_net_phase_inputs at ordering O: x (+-1 of the alpha then the beta bits of model pairs 0..P-2) and occ (the last
    model pair's outcome) exactly as numpy reads them from q2m; the blas training forward and log_psi_train (whose phase
    inputs come from FusedLogPsi._phase_shifts) on top: the amplitude column bit for bit, the phase to 1e-6."""
    from naqs_amd import _lib
    from naqs_amd.hamiltonian import _stream_ptr
    P = gr.sector(name)[1] // 2
    O = ordering(tag, P)
    hil, wfA, wfB, qA, qB = _pair(name, form, O)
    fB = wfB.fused()
    M = min(hil.size, 1000)
    keysB = gr.relabel_keys(gr.random_keys(hil, M, 5), qA, qB)
    k_d = _kdev(keysB)
    x = torch.full((M, 2 * (P - 1)), float("nan"), dtype=torch.float32, device="cuda")
    occ = torch.full((M, 1), -1, dtype=torch.int64, device="cuda")
    _lib.check(fB._lib.naqs_net_phase_inputs(fB._h, M, k_d.data_ptr(), x.data_ptr(), occ.data_ptr(), _stream_ptr(fB.device)),
               "naqs_net_phase_inputs")
    torch.cuda.synchronize()
    bit = lambda q: ((keysB >> np.uint64(q)) & np.uint64(1)).astype(np.int64)
    want_x = np.stack([bit(qB[2 * k]) for k in range(P - 1)] + [bit(qB[2 * k + 1]) for k in range(P - 1)], 1) * 2.0 - 1.0
    want_occ = bit(qB[2 * (P - 1)]) + 2 * bit(qB[2 * (P - 1) + 1])
    assert np.array_equal(x.cpu().numpy(), want_x.astype(np.float32))
    assert np.array_equal(occ.cpu().numpy()[:, 0], want_occ) and len(np.unique(want_occ)) >= 3
    lp_hip, _ = fB.forward_saved(k_d)
    fB.train_mode = "blas"
    try:
        lp_blas, saved = fB.forward_saved(k_d)
        assert saved[1] is not None and torch.equal(saved[1][0], x) and torch.equal(saved[2], occ)
        with torch.no_grad():
            lp_train = fB.log_psi_train(k_d)
    finally:
        fB.train_mode = "hip"
    assert torch.equal(lp_train[:, 0], lp_blas[:, 0])
    assert float((lp_train[:, 1] - lp_blas[:, 1]).abs().max()) <= 1e-6
    assert float((lp_blas[:, 1] - lp_hip[:, 1]).abs().max()) <= 5e-5 and torch.allclose(lp_blas[:, 0], lp_hip[:, 0], rtol=0, atol=2e-6)


# ----------------------------------------------------------------------------------------------------- (c) the sampler
CUTS = [None, ("2", "1", "1"), ("0", "0", "1"), ("1", "1", "4")]       # NAQS_SAMPLE_HEAD / FUSED / MULTI: the three assembly sites
SAMPLER_CASES = [("LiH", "ws", 10 ** 6, 1 << 12), ("LiF", "ws", 10 ** 8, 100000), ("LiH", "deep", 10 ** 6, 1 << 12),
                 ("LiH", "comb", 10 ** 6, 1 << 12)]


def _set_cuts(monkeypatch, cut):
    for k, v in zip(("NAQS_SAMPLE_HEAD", "NAQS_SAMPLE_FUSED", "NAQS_SAMPLE_MULTI"), cut or (None,) * 3):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


@pytest.mark.parametrize("tag", ORDERINGS)
@pytest.mark.parametrize("name,form,n,cap", SAMPLER_CASES)
def test_sampler_draws_the_relabelled_table(name, form, n, cap, tag, monkeypatch):
    """The Philox stream is keyed by the model-order prefix and the level: handles A (-1) and B (O) draw the same tree from
    the same seed, so keys_B == relabel_keys(keys_A) row by row with equal counts, probs and weights, under every launch cut
    (the second draw of each handle is compared, test_pairs_gpu.test_launch_fusions_change_nothing); B's table is in
    (prefix, outcome) order of ITS model pairs, physical, and its probs are exp(2 log|psi|) of the float64 copy; caps M - 1
    and M give the same verdict for both."""
    import test_forward_f64_gpu as tf
    import test_pairs_gpu as tp
    from naqs_amd.nade import MaxBatchSizeExceededError
    tp._threads()
    P = gr.sector(name)[1] // 2
    O = ordering(tag, P)
    hil, wfA, wfB, qA, qB = _pair(name, form, O)
    fA, fB = wfA.fused(), wfB.fused()
    first = None
    for cut in CUTS:
        _set_cuts(monkeypatch, cut)
        outs = []
        for f in (fA, fB):
            f.sample(n, seed=76, max_unique=cap)
            outs.append(f.sample(n, seed=77, max_unique=cap, with_weights=True))
        (ka, ca, pa, wa), (kb, cb, pb, wb) = outs
        kA, kB = ka.cpu().numpy().astype(np.uint64), kb.cpu().numpy().astype(np.uint64)
        assert len(kA) == len(kB) >= min(hil.size, 4) // 2, (cut, len(kA), len(kB))
        assert np.array_equal(kB, gr.relabel_keys(kA, qA, qB)), cut
        assert torch.equal(ca, cb) and torch.equal(pa, pb) and torch.equal(wa, wb), cut
        if first is None:
            first = (kb.clone(), cb.clone(), pb.clone(), wb.clone())
        else:
            assert all(torch.equal(x, y) for x, y in zip(first, (kb, cb, pb, wb))), cut
    _set_cuts(monkeypatch, None)
    # structure and probabilities at ordering O
    k, c, p = first[0].cpu().numpy().astype(np.uint64), first[1].cpu().numpy(), first[2].double().cpu().numpy()
    M = len(k)
    assert np.all(np.diff(gr.model_index(k, qB)) > 0)
    assert M < 3 or not np.all(np.diff(k.astype(np.int64)) > 0)
    assert tp._physical(hil, k) and (c > 0).all() and c.sum() <= n
    assert np.allclose(first[3].cpu().numpy(), c / c.sum(), rtol=1e-15, atol=0)
    _, B64 = gr.f64_copy(wfB)
    lp = gr.log_amp_f64(B64, _states(hil, k))
    L = len(wfB.model.amp_layers[0].linears()) - 1
    rel = np.abs(p / np.exp(2 * lp) - 1)
    bound = 2 * tf._bound_log(lp, P * L) + 8 * P * tf.U32
    print(f"[ordering sampler {name} {form} {tag}] n={n:.0e} {M} unique, {c.sum()} kept  -1 vs {tag}: same draws under {len(CUTS)} "
          f"launch cuts  |probs / exp(2 log|psi|_f64) - 1| {rel.max():.2e} ({(rel / bound).max():.2f} x bound)")
    assert np.all(rel <= bound), (rel.max(), (rel / bound).max())
    # overflow
    for cap2 in (M - 1, M):         # (an earlier level may hold more live prefixes than the last: M itself need not fit)
        got = []
        for f in (fA, fB):
            try:
                got.append(f.sample(n, seed=77, max_unique=cap2))
            except MaxBatchSizeExceededError:
                got.append(None)
        assert (got[0] is None) == (got[1] is None), (cap2, [o is not None for o in got])
        assert cap2 == M or got[0] is None, "a table of M rows fitted a cap of M - 1"
        if got[0] is not None:
            assert np.array_equal(got[1][0].cpu().numpy().astype(np.uint64), k) and torch.equal(got[0][1], got[1][1])


def test_sampler_exact_chi2_at_plus_one():
    """2 10^6 draws at +1 over LiH's whole space against exp(2 log|psi|) of the float64 copy (p > 1e-4, as
    test_distribution_matches_psi_squared); the network is the one whose torch sampler passes the same statistic on the CPU
    (test_qubit_ordering.test_torch_sampler_at_other_orderings)."""
    hil, wf = gr.sector_net("LiH", seed=3, qubit_ordering=1, phase_hidden=(32, 32))
    fused = wf.fused()
    n = 2_000_000
    keys, counts, _ = fused.sample(n, seed=20240607, max_unique=hil.size + 16)
    k, c = keys.cpu().numpy().astype(np.uint64), counts.cpu().numpy()
    all_keys = np.sort(hil._all_keys()).astype(np.uint64)
    pos = np.searchsorted(all_keys, k)
    assert np.array_equal(all_keys[pos], k) and len(np.unique(k)) == len(k) and c.sum() <= n
    obs = np.zeros(len(all_keys))
    obs[pos] = c
    _, wf64 = gr.f64_copy(wf)
    p = np.exp(2 * gr.log_amp_f64(wf64, _states(hil, all_keys)))
    assert abs(c.sum() - n * p.sum()) < 6 * np.sqrt(n * p.sum() * (1 - p.sum())) + 1
    chi2, cells, pv = chi2_pvalue(obs, p)
    print(f"[ordering sampler chi2 LiH +1] n={n:.0e} unique {len(k)} cells {cells} chi2 {chi2:.1f} p-value {pv:.3g}")
    assert pv > PV, (chi2, cells, pv)


# -------------------------------------------------------------------------------------------------------- (d) the step
@pytest.mark.parametrize("name", ["LiH", "LiF"])
def test_library_loop_equals_step_by_step_at_plus_one(name, tmp_path, monkeypatch):
    """naqs_vmc_run over 5 steps against one naqs_vmc_step per step at +1: energies, sample counts, parameters bit for bit."""
    import test_pairs_gpu as tp
    tp._loop_equals_step_by_step(name, tmp_path, monkeypatch, 5, qubit_ordering=1)


@pytest.mark.parametrize("overlap", ["2", "0"])
@pytest.mark.parametrize("name", ["LiH", "LiF"])
def test_forward_after_library_training_steps_at_plus_one(name, overlap, tmp_path, monkeypatch):
    """After 5 library steps at +1 with no refresh: the forward of the whole space against the float64 copy of the current
    parameters (the sampled tables the re-pack rides on are not in ascending key order here)."""
    import test_pairs_gpu as tp
    tp._forward_after_training(name, overlap, tmp_path, monkeypatch, 5, qubit_ordering=1)


def test_cli_run_at_plus_one(tmp_path, capsys):
    """`python -m experiments.run -qo 1` on H2 (the terms of the reference's molecules/H2, packed), 20 steps: the fused path
    (no fallback banner), a finite energy, and no device-side complaint left on the handle (naqs_net_check)."""
    import sys
    import test_pairs_gpu as tp
    from conftest import PKG
    sys.path.insert(0, PKG)
    from experiments import _base
    from naqs_amd import _lib, packing
    mol = str(tmp_path / "H2.npz")
    packing.save_packed(mol, tp._packed("H2")[0])
    made = {}
    real = _base.PartialSamplingOptimizer

    class Spy(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made["opt"] = self

    _base.PartialSamplingOptimizer = Spy
    try:
        res = _base.run(n_hid=64, n_samps=1e5, n_unq_samps_min=2, n_unq_samps_max=1e5,
                        argv=["-m", mol, "-o", str(tmp_path / "run"), "-qo", "1", "-n_train", "20", "-output_freq", "10", "-s", "111"])
    finally:
        _base.PartialSamplingOptimizer = real
    txt = capsys.readouterr().out
    assert "fused HIP network kernels not available" not in txt
    wf = made["opt"].wavefunction
    assert [int(q) for q in wf.qubit2model_permutation] == [0, 1, 2, 3] and made["opt"].n_steps == 20
    fused = wf.fused()
    assert fused is not None
    _lib.check(fused._lib.naqs_net_check(fused._h), "naqs_net_check")
    assert np.isfinite(res[0]["final"]) and np.isfinite(res[0]["eig"]), res[0]
