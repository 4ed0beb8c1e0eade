"""The kernels on the MI355X against float64 on PEAKED networks: the regime of a trained wave function, not of a fresh one.

Every other float64 suite runs a network at or near default initialisation.  test_peaked.py's recipes (grad_reference.anchor /
rebalance / outlier_unit / grown) put 88 .. 99.98 % of |psi|^2 on one determinant, make the logits O(10), spread log|psi| over
-0.04 .. -91, and give one block weights of unequal magnitude.  What only matters there:

(a) forward: log_psi, forward_saved, naqs_net_logamp and naqs_logpsi_eloc's log psi within test_forward_f64_gpu.py's bounds
    (imported) of the float64 copy at anchor B = 3 and 6, -inf where float64 has -inf, the training forward and
    naqs_logpsi_eloc bit for bit, the kernel form asserted per family;
(b) backward: w proportional to the float64 |psi|^2 over the table, seeds loss_grad_f64(e, w) rounded to float32, kink rows
    zeroed; both training-step call forms bit for bit; each tensor within test_backward_gpu.BOUND, or 4 x the committed
    float32-CPU figure of the case where that is larger (test_peaked.backward_bound; at 1 and 17 rows a tensor whose float64
    gradient is below 1e-2 of its terms is measured in units of the terms, test_peaked.tensor_errors); the uncentred Gram
    matrices of the first 64 kink-free rows within test_sr_gpu.C (amplitude: max(C, 4 x float32 PyTorch's figure));
(c) rebalance: W_l, b_l x 2^k and W_{l+1} x 2^-k (k = -24, -8, 8, 24) is the same float32 function bit for bit; the handles'
    log psi, logamp, sampler output and (rescaled) gradient must be torch.equal — true of the f16x2 kernels only if every
    scale is the exact power of two its maximum implies and c, c1, c2 undo it exactly;
(d) outlier_unit: a dead hidden unit R times its neighbours sets a block's sw1 and sh.  R = 2^10: the bounds of (a), (b) and
    the sampler's probs hold; R = 2^16, 2^22: finite, the order of the keys kept, the error printed;
(e) grown: forward and probs as (a); backward within 4 x the float32-CPU figure (test_peaked.GROWN_YARDSTICK);
(f) sampler on a peaked tree: structure, dropped draws, probs, an exact chi-square with the dropped draws as a cell (LiH,
    LiF), the level-by-level test (Li2O, syn32_8_8 — under FULL masking, see test_sampler_levels), 10^12 draws, launch cuts;
(g) the one-call step with M <= 4 unique samples, taken and abandoned.

Rows per table (test_peaked.table): the anchor, the keys of float64 p >= 1e-12 (the 350 largest; the anchor's pair moves where
the space is not enumerated), 200 random keys of the tail, 50 unphysical keys; leading row counts 1, 17, all.

Measured on an MI355X (the whole module: 17 s; profiles/peaked.txt has every case), HIP beside float32 PyTorch on the CPU:
forward 0.37 .. 0.91 of the bound (CPU 0.21 .. 0.76), Li2O and syn32_8_8 at B = 6 1.07 and 1.16 (CPU 0.70, 0.66: held to 4 x
those); backward over all rows 0.03 .. 0.15 of the bound (CPU the same), at 17 rows 7.5e-7 .. 3.2e-6 and, in the nine yardstick cases,
6.7e-6 .. 1.4e-4 (CPU 6.7e-6 .. 1.4e-4: the kernels within 3 % of it); amplitude Gram 9.7e-7 / 1.21e-3 (CPU 1.34e-6 / 1.21e-3);
probs 0.02 .. 0.17 of the bound; rebalance the same bits in 64 of 64 cases; outlier R = 2^10 0.43 .. 0.63 of the forward bound,
R = 2^16 1.5 .. 1.8 x float32 PyTorch, R = 2^22 50 .. 94 x (the format's envelope); chi-square p-values 0.19 .. 0.64 (host:
float32 counts 0.28 .. 0.77, a moved share rejected down to 1e-3 .. 3e-4), level p-values 0.083 and 0.26 pooled, >= 0.034 per
level (host: 0.18, 0.56; 3e-4).
"""
import os

import numpy as np
import pytest
from scipy import stats

import grad_reference as gr
import test_peaked as pk

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PV = 1e-4
U32 = 2.0 ** -24
SEED_DRAW = 20261019


def _threads():
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))


def _kdev(keys):
    return torch.as_tensor(np.asarray(keys).astype(np.int64), device="cuda")


def _dims(wf):
    lin = wf.model.amp_layers[0].linears()
    return lin[0].out_features, len(lin) - 1


def _expect(family, M, save, env, ha, cu):
    """The forward's kernel name per family (test_forward_f64_gpu._expect and its siblings)."""
    import test_amp_depth_gpu as td
    import test_forward_f64_gpu as tf
    if family == "deep2":
        return td._expect(True, M, 2, ha, save=save)
    if family == "aggdeep":
        return f"agg_deep_kernel<{ha // 16}, L=2> + agg_finish_kernel"
    if family == "comb":
        return f"amp_mfma_kernel<{ha // 16}> + comb_head_kernel + comb_finish_kernel"
    kind = {"agg": "agg", "h64": "h", "amp128": "h"}.get(family, "ws")     # (Ha = 128: no amplitude waves beside, phase_kernel_h)
    return tf._expect(kind, M, save, env, ha, cu)


_REF = {}


def _case(name, family, recipe):
    """Per case, computed once and left unchanged: the network on the GPU with its handle, the float64 and float32 CPU copies,
    the key table and both references on it.  One handle serves every NAQS_WS_SPLIT / NAQS_AMP_MODE setting: the library reads
    those on each call (NAQS_PHASE_MODE, read when the weights are packed, is set only by test_rebalance, which builds its own)."""
    key = (name, family, recipe)
    if key not in _REF:
        _threads()
        hil, wf, anchor, touched = pk.peaked(name, family, recipe, device="cuda")
        fused = wf.fused()
        assert fused is not None and fused.train_mode == "hip"
        _, wf64 = gr.f64_copy(wf)
        _, wf32 = gr.f64_copy(wf, dtype=torch.float32)
        keys, n_phys = pk.table(hil, wf64, anchor)
        st = pk.states(hil, keys)
        ref64, ref32 = gr.log_psi_f64(wf64, st), gr.log_psi_f64(wf32, st)
        assert not np.isnan(ref64).any() and np.isfinite(ref64[:n_phys, 0]).all()
        _REF[key] = dict(hil=hil, wf=wf, fused=fused, wf64=wf64, wf32=wf32, anchor=anchor, touched=touched, keys=keys,
                         n_phys=n_phys, ref64=ref64, ref32=ref32)
    return _REF[key]


def _logamp(fused, k_d):
    from naqs_amd import _lib
    from naqs_amd.hamiltonian import _stream_ptr
    la = torch.full((k_d.shape[0],), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(fused._lib.naqs_net_logamp(fused._h, k_d.shape[0], k_d.data_ptr(), la.data_ptr(), _stream_ptr(fused.device)),
               "naqs_net_logamp")
    return la


# --------------------------------------------------------------------------------------------------------- (a) forward
def _check_forward(tag, r, family, env, ham=None, factor=1.0):
    """-> (problems, worst HIP error / bound, worst float32-CPU error / bound) over the leading row counts 1, 17, all.
    ``factor``: the log|psi| bound's multiple where float32 PyTorch itself uses most of it (test_peaked.FORWARD_YARDSTICK)."""
    import test_forward_f64_gpu as tf
    import test_pairs_gpu as tp
    cu = tf._cus()
    hil, fused, keys = r["hil"], r["fused"], r["keys"]
    ha, L = _dims(r["wf"])
    P = hil.N // 2
    scale = np.abs(r["ref64"][:, 1]).max()
    fails, worst, worst32 = [], 0.0, 0.0
    for m in (1, 17, len(keys)):
        ks, want, want32 = gr.sorted_rows(keys, m, r["ref64"], r["ref32"])
        k_d = _kdev(ks)
        lp = fused.log_psi(k_d).clone()
        ran = fused.last_kernel().split(";")[0]
        bad, e0, e1, rr = tp._compare(lp.cpu().numpy(), want, P * L, scale)
        _, c0, c1, r32 = tp._compare(want32, want, P * L, scale)
        if factor > 1:
            bad = [b for b in bad if not b.startswith("log|psi|")] + ([f"log|psi| {e0:.2e} ({rr:.2f} x bound)"] if not rr <= factor else [])
        if ran != _expect(family, m, 0, env, ha, cu):
            bad.append(f"ran {ran!r}, expected {_expect(family, m, 0, env, ha, cu)!r}")
        if env.get("NAQS_PHASE_MODE") != "0":
            lpt, _ = fused.forward_saved(k_d)
            if not torch.equal(lpt, lp):
                bad.append("forward_saved differs from naqs_net_logpsi")
            if fused.last_kernel().split(";")[0] != _expect(family, m, 1, env, ha, cu):
                bad.append(f"training forward ran {fused.last_kernel()!r}")
        la = _logamp(fused, k_d).double().cpu().numpy()
        fin = np.isfinite(want[:, 0])
        r_la = (np.abs(la[fin] - want[fin, 0]) / tf._bound_log(want[fin, 0], P * L)).max(initial=0.0)
        if not r_la <= factor or not np.array_equal(la == -np.inf, ~fin) or np.isnan(la).any():
            bad.append(f"naqs_net_logamp {r_la:.2f} x bound")
        if ham is not None and fin.any():
            kp = _kdev(ks[fin])
            lp_p = fused.log_psi(kp).clone()
            lp_e, e_loc = fused.log_psi_and_local_energy(ham, kp)
            torch.cuda.synchronize()
            if not torch.equal(lp_e, lp_p) or not bool(torch.isfinite(e_loc).all()):
                bad.append("naqs_logpsi_eloc's log psi differs from naqs_net_logpsi")
        worst, worst32 = max(worst, rr, r_la), max(worst32, r32)
        print(f"[peaked forward {tag}] M={m:4d} {ran}  |HIP - f64| log {e0:.2e} phase {e1:.2e} ({rr:.2f} x bound, logamp "
              f"{r_la:.2f})  |torch f32 CPU - f64| log {c0:.2e} phase {c1:.2e} ({r32:.2f} x bound)  -inf rows {int((~fin).sum())}")
        fails += [(m, b) for b in bad]
    return fails, worst, worst32


FORWARD = [("LiH", "ws", {}), ("LiH", "ws", {"NAQS_WS_SPLIT": "0"}), ("LiH", "ws", {"NAQS_AMP_MODE": "2"}),
           ("LiH", "ws", {"NAQS_AMP_MODE": "0"}), ("LiF", "ws", {}), ("Li2O", "ws", {}), ("syn32_8_8", "ws", {}), ("O2", "ws", {}),
           ("LiH", "h64", {}), ("LiF", "h64", {}), ("LiH", "amp32", {"NAQS_AMP_MODE": "2"}), ("LiH", "amp128", {}),
           ("LiF", "agg", {}), ("LiH", "aggdeep", {}), ("LiH", "deep2", {}), ("LiH", "comb", {})]


def _ham(name):
    import test_pairs_gpu as tp
    from naqs_amd import hamiltonian
    return hamiltonian.DevicePauliHamiltonian(tp._row_ham(name, None), device="cuda:0")


def _ids(v):
    return v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items()) or "default"


@pytest.mark.parametrize("name,family,env", FORWARD, ids=_ids)
def test_forward_against_float64(name, family, env, monkeypatch):
    import test_forward_f64_gpu as tf
    tf._set_env(monkeypatch, env)
    ham = _ham(name) if (name, family) in (("LiH", "ws"), ("LiF", "ws"), ("LiF", "agg")) and not env else None
    fails = []
    for B in (3, 6):
        r = _case(name, family, ("anchor", B))
        # (a failure inside 4 x the float32-CPU error on the same rows is the bound model, not the kernel: logits O(B))
        factor = max(1.0, 4 * pk.FORWARD_YARDSTICK.get((name, B), 0.0)) if family == "ws" else 1.0
        f, worst, worst32 = _check_forward(f"{name} {family} {env or ''} B={B}", r, family, env, ham, factor)
        print(f"[peaked forward {name} {family} {env or ''} B={B}] worst HIP {worst:.2f} x bound, torch f32 CPU {worst32:.2f} x bound")
        fails += [(B,) + x for x in f]
    assert not fails, fails


# -------------------------------------------------------------------------------------------------------- (b) backward
def _check_backward(tag, r, case, tau=pk.TAU, gram=None, seed=11):
    """``case`` = (name, family, recipe): the per-tensor bound is test_backward_gpu.BOUND, or 4 x the committed float32-CPU
    figure of the case where that is larger (test_peaked.backward_bound: the grown tables, and 17-row tables whose
    float32-CPU figure exceeds a quarter of BOUND).  -> (problems, worst HIP / bound, worst float32 CPU / bound)."""
    import test_backward_gpu as tb
    hil, wf, fused, wf64, wf32 = r["hil"], r["wf"], r["fused"], r["wf64"], r["wf32"]
    phys = r["keys"][:r["n_phys"]]
    fails, worst, worst32 = [], 0.0, 0.0
    for m in (1, 17, len(phys)):
        ks = np.sort(phys[:m])
        bound = pk.backward_bound(*case, rows17=m <= 17)
        e, w, g, margin, lp = pk.backward_case(hil, wf64, ks, tau, seed)
        k_d, e_d, w_d, s_d = _kdev(ks), tb._dev(tb._c2(e)), tb._dev(w), tb._dev(tb._sums(e, w))
        # the two training-step call forms
        tb._zero_grad(wf)
        fused._grad_flat = None
        _, saved = fused.forward_saved(k_d)
        g1, ev1 = fused.backward_from_local_energy(saved, e_d, w_d, s_d)
        got1 = tb._grads(wf)
        tb._zero_grad(wf)
        fused._grad_flat = None
        _, saved = fused.forward_saved(k_d)
        g2 = fused.vmc_loss_grad(e_d, w_d, s_d)
        fused.backward_saved(saved, g2)
        got2 = tb._grads(wf)
        same = torch.equal(g1, g2) and all(np.array_equal(got1[n], got2[n]) for n in got1)
        # (the loss-gradient kernel rounds E and <E> to float32 before their difference: test_backward_gpu.py's bound (b);
        # + one float32 rounding of the reference seeds themselves)
        gk, u, mean = g1.double().cpu().numpy(), U32, (w * e).sum()
        gb = np.stack([2 * w * ((np.abs(e.real) + abs(mean.real)) * u + np.abs(e.real - mean.real) * 3 * u),
                       2 * w * ((np.abs(e.imag) + abs(mean.imag)) * u + np.abs(e.imag - mean.imag) * 3 * u)], -1) * (1 + 4 * u)
        # (the tail's weights go down to 1e-43: below float32's normal range a seed is a subnormal, or flushed — 2^-126 absolute)
        if not np.all(np.abs(gk - g) <= gb + u * np.abs(g) + 1e-15 * 2 * w[:, None] * abs(mean) + 2.0 ** -126):
            fails.append((m, "vmc_loss_grad is not loss_grad_f64", float(np.max(np.abs(gk - g)))))
        # the seeds of the float64 formula, rounded to float32
        tb._zero_grad(wf)
        fused._grad_flat = None
        _, saved = fused.forward_saved(k_d)
        fused.backward_saved(saved, tb._dev(g, torch.float32))
        got = tb._grads(wf)
        torch.cuda.synchronize()
        want = gr.grad_f64(wf64, None, g, lp=lp)
        want32 = gr.grad_f64(wf32, pk.states(hil, ks), g.astype(np.float32))
        st = pk.states(hil, ks)
        errs, by_terms = pk.tensor_errors(wf64, st, g, got, want, r["touched"], m <= 17)
        e32s, _ = pk.tensor_errors(wf64, st, g, want32, want, r["touched"], m <= 17)
        e32 = max(e32s.values())
        e_hip = max(errs.values())
        worst, worst32 = max(worst, e_hip / bound), max(worst32, e32 / bound)
        print(f"[peaked backward {tag}] M={m:4d} kink rows {int((margin < tau).sum()):3d}  |HIP - f64| {e_hip:.2e} "
              f"({e_hip / bound:.2f} x bound)  |torch f32 CPU - f64| {e32:.2e}  call forms {'same bits' if same else 'DIFFER'}"
              + (f"  ({by_terms} cancelling tensors in units of their terms)" if by_terms else ""))
        if not same:
            fails.append((m, "the two call forms differ"))
        fails += [(m, n, v) for n, v in errs.items() if not v <= bound]
    if gram:
        import sr_reference as sr
        from test_sr_gpu import C
        ks = pk.gram_rows(hil, wf64, phys)
        A, B = sr.jacobians(wf64, pk.states(hil, ks))
        _, saved = fused.forward_saved(_kdev(ks))
        Ga, Gp = fused.sr_gram(saved, None, None, None, uncentred=True)
        torch.cuda.synchronize()
        ea, ep = sr.gram_err(Ga.cpu().numpy(), A @ A.T), sr.gram_err(Gp.cpu().numpy(), B @ B.T)
        # (the anchor's row is d log|psi| = onehot - softmax with softmax = 1 - e^-2B: float32 keeps 2^-24 / (1 - p) of it, in
        # PyTorch as in the kernels — the amplitude bound is max(C, 4 x the float32-CPU figure of the same rows))
        Ca = max(C, 4 * gram)
        print(f"[peaked gram {tag}] M={len(ks)}  |G - G64| amplitude {ea:.2e} (bound {Ca:.2e}, torch f32 CPU {gram:.2e}) phase {ep:.2e} "
              f"(bound {C:.2e})")
        if not (ea <= Ca and ep <= C):
            fails.append(("gram", ea, ep))
    return fails, worst, worst32


# the networks and forced kernel forms of FORWARD (the training forward saves what the backward reads)
BACKWARD = FORWARD


@pytest.mark.parametrize("name,family,env", BACKWARD, ids=_ids)
def test_backward_against_float64(name, family, env, monkeypatch):
    import test_forward_f64_gpu as tf
    tf._set_env(monkeypatch, env)
    fails = []
    for B in (3, 6):
        r = _case(name, family, ("anchor", B))
        f, worst, worst32 = _check_backward(f"{name} {family} {env or ''} B={B}", r, (name, family, ("anchor", B)),
                                            gram=pk.GRAM_YARDSTICK.get((name, family, B)) if not env else None)
        print(f"[peaked backward {name} {family} {env or ''} B={B}] worst HIP {worst:.2f} x bound, torch f32 CPU {worst32:.2f} x bound")
        fails += [(B,) + x for x in f]
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------- (c) rebalance
F32_ENV = {"NAQS_AMP_MODE": "0", "NAQS_PHASE_MODE": "0", "NAQS_SAMPLE_MFMA": "0"}     # the f32 forms: the control
REBALANCE = [(f, False) for f in pk.PARTS] + [("ws", True)]


def _everything(wf, keys_all, keys_phys, g, grads):
    fused = wf.fused()
    assert fused is not None
    import test_backward_gpu as tb
    out = {"log_psi": fused.log_psi(_kdev(keys_all)).clone(), "logamp": _logamp(fused, _kdev(keys_all))}
    for i, t in enumerate(fused.sample(10 ** 6, seed=SEED_DRAW, max_unique=1 << 16)):
        out[("keys", "counts", "probs")[i]] = t.clone()
    if grads:
        tb._zero_grad(wf)
        fused._grad_flat = None
        _, saved = fused.forward_saved(_kdev(keys_phys))
        fused.backward_saved(saved, g)
        out["grad"] = {n: p.grad.detach().clone() for n, p in wf.model.named_parameters()}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("family,f32", REBALANCE, ids=lambda v: v if isinstance(v, str) else ("f32" if v else "f16x2"))
def test_rebalance_gives_the_same_bits(family, f32, monkeypatch):
    """LiH, anchor(3): for every part and k the rebalanced handle's log psi (both columns), logamp, sampler output and
    gradient (the two rescaled tensors' times 2^k and 2^-k: exact) are torch.equal to the k = 0 handle's.  The f32 control
    has no gradient part: phase_kernel (NAQS_PHASE_MODE=0) saves no activations, so there is no training forward under it."""
    import test_backward_gpu as tb
    for k_, v in (F32_ENV if f32 else {}).items():
        monkeypatch.setenv(k_, v)
    r = _case("LiH", family, ("anchor", 3))
    hil = r["hil"]
    keys_all = np.sort(r["keys"])
    keys_phys = np.sort(r["keys"][:r["n_phys"]])
    _, _, g, _, _ = pk.backward_case(hil, r["wf64"], keys_phys)
    g_d = tb._dev(g, torch.float32)
    _, wf0, _, _ = pk.peaked("LiH", family, ("anchor", 3), device="cuda")          # (built under this test's environment)
    base = _everything(wf0, keys_all, keys_phys, g_d, not f32)
    assert len(base["keys"]) >= 10 and torch.isfinite(base["log_psi"][:, 1]).all()
    fails = []
    for part in pk.PARTS[family]:
        for k in pk.KS:
            _, wf, _, _ = pk.peaked("LiH", family, ("anchor", 3), device="cuda")
            up, down = gr.rebalance(wf, k, part)
            out = _everything(wf, keys_all, keys_phys, g_d, not f32)
            diff = [n for n in ("log_psi", "logamp", "keys", "counts", "probs") if not torch.equal(out[n], base[n])]
            if not f32:
                for n, gb in base["grad"].items():
                    f = 2.0 ** k if n in up else 2.0 ** -k if n in down else 1.0
                    if not torch.equal(out["grad"][n] * f, gb):
                        d = float((out["grad"][n] * f - gb).abs().max() / gb.abs().max().clamp_min(1e-30))
                        diff.append(f"grad {n} ({d:.1e})")
            print(f"[peaked rebalance LiH {family} {'f32' if f32 else 'f16x2'}] {part} k={k:+d}: {'same bits' if not diff else diff}")
            if diff:
                fails.append((part, k, diff))
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------- (d) outlier_unit
def _check_probs(tag, r, n=10 ** 6):
    import test_forward_f64_gpu as tf
    hil, fused = r["hil"], r["fused"]
    _, L = _dims(r["wf"])
    keys, counts, probs = fused.sample(n, seed=SEED_DRAW, max_unique=1 << 20)
    k, c, p = keys.cpu().numpy().astype(np.uint64), counts.cpu().numpy(), probs.double().cpu().numpy()
    assert len(k) >= 1 and np.all(np.diff(k) > 0) and hil.is_physical(k).all() and (c > 0).all() and c.sum() <= n
    st = pk.states(hil, k)
    lp, lp32 = gr.log_amp_f64(r["wf64"], st), gr.log_amp_f64(r["wf32"], st)
    P = hil.N // 2
    bound = 2 * tf._bound_log(lp, P * L) + 8 * P * U32
    rel, rel32 = np.abs(p / np.exp(2 * lp) - 1), np.abs(np.exp(2 * (lp32 - lp)) - 1)
    print(f"[peaked probs {tag}] {len(k)} unique, {c.sum()} kept of {n}  |probs / exp(2 log|psi|_f64) - 1| {rel.max():.2e} "
          f"({(rel / bound).max():.2f} x bound)  torch f32 CPU {rel32.max():.2e} ({(rel32 / bound).max():.2f} x bound)")
    return [] if np.all(rel <= bound) else [("probs", float(rel.max()), float((rel / bound).max()))]


OUTLIER = [("LiH", "ws"), ("LiF", "ws"), ("LiH", "amp128"), ("LiF", "agg"), ("LiH", "deep2")]


@pytest.mark.parametrize("name,family", OUTLIER)
def test_outlier_unit_within_the_bounds_at_2_10(name, family):
    """R = 2^10: sh h of an ordinary unit is still >= 2^-2, where the low f16 plane keeps 2^-23 of the value (hi 11 bits, lo
    quantum 2^-24): forward, probs and backward (the dead unit's own rows left out of the per-tensor maxima) as in (a), (b)."""
    r = _case(name, family, ("outlier", 2.0 ** 10))
    tag = f"{name} {family} R=2^10"
    fails, w, w32 = _check_forward(tag, r, family, {})
    fails += _check_probs(tag, r)
    fb, wb, wb32 = _check_backward(tag, r, (name, family, ("outlier", 2.0 ** 10)))
    print(f"[peaked outlier {tag}] forward {w:.2f} x bound (f32 CPU {w32:.2f}), backward {wb:.2f} x bound (f32 CPU {wb32:.2f})")
    assert not fails + fb, fails + fb


@pytest.mark.parametrize("name,family", OUTLIER[:3])
@pytest.mark.parametrize("e", [16, 22])
def test_outlier_unit_past_the_envelope_stays_finite(name, family, e):
    """R = 2^16, 2^22: finite, -inf only where float64 has it, and the order of the table's keys by log|psi| kept wherever
    float64 separates two neighbours by more than 1e-2; the error is printed beside float32 PyTorch's (the format's
    envelope: profiles/peaked.txt, DESIGN)."""
    import test_forward_f64_gpu as tf
    r = _case(name, family, ("outlier", 2.0 ** e))
    ks, want, want32 = gr.sorted_rows(r["keys"], len(r["keys"]), r["ref64"], r["ref32"])
    lp = r["fused"].log_psi(_kdev(ks)).double().cpu().numpy()
    fin = np.isfinite(want[:, 0])
    assert not np.isnan(lp).any() and np.array_equal(lp[:, 0] == -np.inf, ~fin) and np.isfinite(lp[fin]).all()
    order = np.argsort(want[fin, 0])
    a, b = want[fin, 0][order], lp[fin, 0][order]
    sep = np.diff(a) > 1e-2
    assert np.all(np.diff(b)[sep] > 0)
    P = r["hil"].N // 2
    bound = tf._bound_log(want[fin, 0], P * _dims(r["wf"])[1])
    e_hip, e_32 = np.abs(lp[fin, 0] - want[fin, 0]), np.abs(want32[fin, 0] - want[fin, 0])
    print(f"[peaked outlier {name} {family} R=2^{e}] |HIP - f64| log {e_hip.max():.2e} ({(e_hip / bound).max():.2f} x bound)  "
          f"|torch f32 CPU - f64| {e_32.max():.2e} ({(e_32 / bound).max():.2f} x bound)  HIP / f32 CPU {e_hip.max() / e_32.max():.1f}")


# ----------------------------------------------------------------------------------------------------------- (e) grown
@pytest.mark.parametrize("name,family", list(pk.GROWN_YARDSTICK))
def test_grown_network(name, family):
    r = _case(name, family, ("grown",))
    tag = f"{name} {family} grown"
    fails, w, w32 = _check_forward(tag, r, family, {})
    fails += _check_probs(tag, r)
    fb, wb, wb32 = _check_backward(tag, r, (name, family, ("grown",)), tau=pk.TAU * pk.GROWN_HIDDEN, seed=pk.GROWN_SEED)
    print(f"[peaked grown {tag}] forward {w:.2f} x bound (f32 CPU {w32:.2f}), backward {wb:.2f} x bound = 4 x f32 CPU yardstick")
    assert not fails + fb, fails + fb


# --------------------------------------------------------------------------------------------------------- (f) sampler
SHARES = [1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5]


def _cells_chi2(obs, dropped, p, n):
    """Exact chi-square of one draw of n: every key with n p >= 10 its own cell, the other physical keys one pooled cell,
    the dropped draws one cell (p: float64 probability of every physical key; they sum to less than 1 under PARTIAL masking).
    -> (chi2, cells, p-value)."""
    own = n * p >= 10
    o = np.r_[obs[own], obs[~own].sum(), dropped]
    e = np.r_[n * p[own], n * p[~own].sum(), n * (1 - p.sum())]
    keep = e > 0
    chi2 = ((o[keep] - e[keep]) ** 2 / e[keep]).sum()
    assert o[~keep].sum() == 0
    return chi2, int(keep.sum()), stats.chi2.sf(chi2, keep.sum() - 1)


# (network, n, the smallest moved share of the anchor's root conditional the host check must reject at that n)
CHI2 = [("LiH", "ws", 10 ** 7, 1e-3), ("LiF", "ws", 10 ** 8, 3e-4), ("LiH", "deep2", 10 ** 7, 3e-4), ("LiH", "amp128", 10 ** 7, 1e-3)]


@pytest.mark.parametrize("name,family,n,share", CHI2)
def test_sampler_exact_chi2(name, family, n, share):
    """anchor(3) over the enumerated space under PARTIAL masking: keys ascending, unique, physical; the dropped draws within
    5 sigma of Binomial(n, 1 - sum p64); probs against exp(2 log|psi|_f64); the chi-square of _cells_chi2.  Host checks with
    numpy at the same n: counts drawn from the float32-CPU network's probabilities pass (float32 rounding is not what the
    test sees), counts drawn from float64 with a share of the anchor's root conditional moved to its smallest sibling are
    rejected — every share from 1e-2 down to CHI2's (1e-3 on LiH's published shape and Ha = 128, 3e-4 on LiF and the deep net)."""
    import test_forward_f64_gpu as tf
    r = _case(name, family, ("anchor", 3))
    hil, fused = r["hil"], r["fused"]
    _, L = _dims(r["wf"])
    keys, counts, probs = fused.sample(n, seed=SEED_DRAW, max_unique=hil.size + 16)
    k, c, pr = keys.cpu().numpy().astype(np.uint64), counts.cpu().numpy(), probs.double().cpu().numpy()
    assert np.all(np.diff(k) > 0) and hil.is_physical(k).all() and (c > 0).all() and c.sum() <= n
    allk = pk.whole(hil)
    st = pk.states(hil, allk)
    lp64, lp32 = gr.log_amp_f64(r["wf64"], st), gr.log_amp_f64(r["wf32"], st)
    p, p32 = np.exp(2 * lp64), np.exp(2 * lp32)
    pos = np.searchsorted(allk, k)
    assert np.array_equal(allk[pos], k)
    P = hil.N // 2
    rel = np.abs(pr / p[pos] - 1)
    bound = 2 * tf._bound_log(lp64[pos], P * L) + 8 * P * U32
    q = 1 - p.sum()
    dropped = n - c.sum()
    z = (dropped - n * q) / np.sqrt(n * q * (1 - q))
    obs = np.zeros(len(allk))
    obs[pos] = c
    chi2, cells, pv = _cells_chi2(obs, dropped, p, n)
    # host checks
    rs = np.random.RandomState(3)
    d32 = rs.multinomial(n, np.r_[p32, max(1 - p32.sum(), 0)] / (p32.sum() + max(1 - p32.sum(), 0)))
    pv32 = _cells_chi2(d32[:-1].astype(float), d32[-1], p, n)[2]
    p0, phys0 = gr.conditionals_f64(r["wf64"], st[:1], 0)
    p0, phys0 = p0[0], phys0[0]
    order = [j for j in np.argsort(-p0) if phys0[j]]
    ms = st[:, r["wf64"]._q2m.cpu()]
    child0 = ((ms[:, 0] > 0).long() + 2 * (ms[:, 1] > 0).long()).numpy()
    assert child0[np.searchsorted(allk, r["anchor"])] == order[0]
    rejected = []
    for s in SHARES:
        moved = _moved(p0, order[0], order[-1], s)
        pm = p * (moved / np.where(p0 > 0, p0, 1))[child0]
        dm = rs.multinomial(n, np.r_[pm, 1 - pm.sum()])
        if _cells_chi2(dm[:-1].astype(float), dm[-1], p, n)[2] < PV:
            rejected.append(s)
    print(f"[peaked chi2 {name} {family}] n={n:.0e} space {hil.size} unique {len(k)} cells {cells} chi2 {chi2:.1f} p-value {pv:.3g}  "
          f"dropped {dropped} ({z:+.2f} sigma of Binomial(n, {q:.4f}))  probs {(rel / bound).max():.2f} x bound  host: float32 "
          f"counts p-value {pv32:.3g}, rejects a moved share down to {min(rejected) if rejected else 'NONE'}")
    assert np.all(rel <= bound), (rel.max(), (rel / bound).max())
    assert abs(z) <= 5, z
    assert pv > PV, (chi2, cells, pv)
    assert pv32 > PV, "float32 rounding alone fails the chi-square at this n"
    assert [s for s in SHARES if s >= share] == rejected[:len([s for s in SHARES if s >= share])], (share, rejected)


def _moved(p, src, dst, share):
    q = p.copy()
    q[src] -= share * p[src]
    q[dst] += share * p[src]
    return q


@pytest.mark.parametrize("name", ["Li2O", "syn32_8_8"])
def test_sampler_levels(name):
    """anchor(3), 10^6 draws, spaces too large to enumerate: every node's children counts against Multinomial(count, float64
    conditionals), level by level (grad_reference.tree_chi2; a node's children of expectation < 5 pooled, nodes left with one
    cell skipped; a pooled cell expecting less than one draw — Cochran's rule — joins the node's smallest cell of >= 5).  Under FULL masking: with PARTIAL masking the draws that end unphysical are dropped at the last pair, and
    what survives is, at every level above, weighted by each subtree's survival — not Multinomial(p) (the enumerated spaces
    of test_sampler_exact_chi2 carry PARTIAL masking's dropped draws as a cell; here the same network's probs and structure
    are checked under PARTIAL masking as well).  Nodes with two or more physical children that are skipped may hold at most
    1 % of their level's draws (a node whose budget leaves one child has nothing to test).  Host checks: the torch sampler's
    draws from the float32-CPU network pass; the anchor's conditional at the first level, with a share moved to its
    smallest sibling, is rejected by that level at every share from 1e-2 down to 3e-4."""
    rp = _case(name, "ws", ("anchor", 3))
    fails = _check_probs(f"{name} ws PARTIAL", rp)
    _threads()
    hil, wf, anchor, _ = pk.peaked(name, "ws", ("anchor", 3), device="cuda", masking="FULL")
    fused = wf.fused()
    _, wf64 = gr.f64_copy(wf)
    _, wf32 = gr.f64_copy(wf, dtype=torch.float32)
    n = 10 ** 6
    keys, counts, _ = fused.sample(n, seed=SEED_DRAW, max_unique=1 << 20)
    k, c = keys.cpu().numpy().astype(np.uint64), counts.cpu().numpy()
    assert c.sum() == n and np.all(np.diff(k) > 0) and hil.is_physical(k).all()
    assert c[np.searchsorted(k, anchor)] > 0.88 * n
    P = hil.N // 2
    tree = gr.tree_levels(wf64, hil, k, c)

    chi2, dof, pv, levels, masked, skipped = gr.tree_chi2(tree, min_lump=1)
    # host: the torch sampler on the float32 CPU copy
    gen = torch.Generator().manual_seed(5)
    from naqs_amd.nade import NadeMasking
    st32, c32, _ = wf32.model._forward_sample(n, ret_output=False, masking=NadeMasking.FULL, generator=gen)
    inv = torch.argsort(wf32._q2m.cpu())
    k32 = hil.state2idx(st32[:, inv]).reshape(-1).numpy().astype(np.uint64)
    o32 = np.argsort(k32)
    _, _, pv32, lv32, _, _ = gr.tree_chi2(gr.tree_levels(wf64, hil, k32[o32], c32.numpy()[o32]), min_lump=1)
    p0, phys0 = gr.conditionals_f64(wf64, pk.states(hil, k[:1]), 0)
    order = [j for j in np.argsort(-p0[0]) if phys0[0][j]]
    rejected = [s for s in SHARES if gr.tree_chi2(tree, root=_moved(p0[0], order[0], order[-1], s), min_lump=1)[3][0] < PV / P]
    print(f"[peaked levels {name}] n={n} unique {len(k)} anchor {c[np.searchsorted(k, anchor)] / n:.3f}  chi2 {chi2:.1f} dof {dof} "
          f"p-value {pv:.3g}  level p-values {' '.join('%.2g' % v for v in levels)}  skipped share {max(skipped):.2e}  host: "
          f"float32 draws p-value {pv32:.3g} (levels >= {min(lv32):.2g}), rejects a moved share down to "
          f"{min(rejected) if rejected else 'NONE'}")
    assert masked == 0 and max(skipped) <= 0.01, (masked, skipped)
    assert pv > PV and min(levels) > PV / P, (pv, levels)
    assert pv32 > PV and min(lv32) > PV / P, "float32 rounding alone fails the level test at this n"
    assert rejected[:4] == SHARES[:4], rejected
    assert not fails, fails


def test_sampler_ten_to_the_twelve_draws():
    """anchor(6) on LiH, 10^12 draws — float32 rounding of the conditionals is visible at this n, so only: sum(counts) <= n in
    int64, the anchor's share within the probs bound plus 6 sigma of its float64 probability, the same bits on a second call."""
    import test_forward_f64_gpu as tf
    r = _case("LiH", "ws", ("anchor", 6))
    hil, fused = r["hil"], r["fused"]
    n = 10 ** 12
    a = fused.sample(n, seed=SEED_DRAW, max_unique=1 << 12)
    b = fused.sample(n, seed=SEED_DRAW, max_unique=1 << 12)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    k, c = a[0].cpu().numpy().astype(np.uint64), a[1].cpu().numpy()
    assert c.dtype == np.int64 and (c > 0).all() and 0 < int(c.sum()) <= n and np.all(np.diff(k) > 0) and hil.is_physical(k).all()
    lp = gr.log_amp_f64(r["wf64"], pk.states(hil, [r["anchor"]]))[0]
    p = np.exp(2 * lp)
    share = c[np.searchsorted(k, r["anchor"])] / n
    P = hil.N // 2
    bound = (2 * tf._bound_log(lp, P) + 8 * P * U32) * p + 6 * np.sqrt(p * (1 - p) / n)
    print(f"[peaked 1e12 LiH] unique {len(k)} kept {c.sum()}  anchor share {share:.9f} vs p64 {p:.9f}: {abs(share - p):.2e} "
          f"({abs(share - p) / bound:.2f} x bound)")
    assert abs(share - p) <= bound


@pytest.mark.parametrize("name", ["LiH", "Li2O"])
def test_launch_cuts_draw_the_same_bits(name, monkeypatch):
    """Every launch cut test_pairs_gpu.FUSIONS switches (head of 5 / 4 / no levels, fused or split levels, 1..4 levels per
    launch), on a tree of a handful of live prefixes per level."""
    from test_pairs_gpu import FUSIONS
    r = _case(name, "ws", ("anchor", 3))
    fused = r["fused"]
    n = 10 ** 7 if name == "LiH" else 10 ** 6
    outs = []
    for head, fuse, multi in FUSIONS:
        monkeypatch.setenv("NAQS_SAMPLE_HEAD", head)
        monkeypatch.setenv("NAQS_SAMPLE_FUSED", fuse)
        monkeypatch.setenv("NAQS_SAMPLE_MULTI", multi)
        outs.append(tuple(t.clone() for t in fused.sample(n, seed=SEED_DRAW + 1, max_unique=1 << 20)))
    for k_ in ("NAQS_SAMPLE_HEAD", "NAQS_SAMPLE_FUSED", "NAQS_SAMPLE_MULTI"):
        monkeypatch.delenv(k_)
    print(f"[peaked launch cuts {name}] n={n} unique {len(outs[0][0])}")
    assert len(outs[0][0]) >= 4
    for f, o in zip(FUSIONS[1:], outs[1:]):
        assert all(torch.equal(x, y) for x, y in zip(outs[0], o)), (name, f)


# ------------------------------------------------------------------------------------------------- (g) the one-call step
ADAM = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-15)


def _step_net(B=6):
    from naqs_amd.flat_adam import FlatAdam
    hil, wf, anchor, _ = pk.peaked("LiH", "ws", ("anchor", B), device="cuda")
    flat = wf.flatten_parameters()
    adam = FlatAdam(wf.param_list(), flat, **ADAM)
    return hil, wf, wf.fused(), adam


def _one_call_against_parts(ham, n, seed, cap, B=6):
    """-> M.  The parts on one network, naqs_vmc_step (abandoned with m_lo = 10, then taken with m_lo = 1) on its twin."""
    hil, wf, fused, adam = _step_net(B)
    k2, c2, p2, w2 = fused.sample(n, seed, cap, with_weights=True)
    M = len(k2)
    assert 1 <= M <= 4, M
    lp2, saved2, eloc2, sums2 = fused.forward_saved_with_local_energy(ham, k2, w2)
    for p in wf.model.parameters():
        p.grad = None
    g2, ev2 = fused.backward_from_local_energy(saved2, eloc2, w2.contiguous(), sums2)
    grad2 = torch.cat([p.grad.reshape(-1) for p in wf.param_list()]).clone()
    adam.step()
    fused.refresh()
    torch.cuda.synchronize()
    allk = _kdev(pk.whole(hil))
    after2 = fused.log_psi(allk).clone()
    hil, wf1, fused1, adam1 = _step_net(B)
    flat0 = wf1.flatten_parameters().clone()
    taken, m0, overflow, _ = fused1.vmc_step(ham, n, seed, cap, 10, cap, adam=adam1)
    torch.cuda.synchronize()
    assert not taken and m0 == M and not overflow                       # (info_host[2] == 0)
    assert torch.equal(wf1.flatten_parameters(), flat0) and adam1._t == 0
    assert not adam1._m.any() and not adam1._v.any()
    taken, m1, overflow, out = fused1.vmc_step(ham, n, seed, cap, 1, cap, adam=adam1)
    torch.cuda.synchronize()
    assert taken and m1 == M and not overflow
    keys, counts, probs, weights, log_psi, eloc, sums, g, ev = out
    for a, b, what in ((keys, k2, "keys"), (counts, c2, "counts"), (probs, p2, "probs"), (weights, w2, "weights"), (log_psi, lp2, "log psi"),
                       (eloc, eloc2, "E_loc"), (sums, sums2, "sums"), (g, g2, "g"), (ev, ev2, "ev"), (fused1._grad_flat, grad2, "gradient"),
                       (wf1.flatten_parameters(), wf.flatten_parameters(), "parameters"), (adam1._m, adam._m, "exp_avg"),
                       (adam1._v, adam._v, "exp_avg_sq")):
        assert torch.equal(a, b), (what, seed, M)
    assert adam1._t == 1 and torch.isfinite(wf1.flatten_parameters()).all()
    if M >= 2:                                                          # (one sample: E_loc - <E> = 0, the step moves nothing)
        assert not torch.equal(wf1.flatten_parameters(), flat0)
    assert torch.equal(fused1.log_psi(allk), after2), "the re-packed weights differ from set_weights of the updated parameters"
    print(f"[peaked one-call step LiH B={B}] n={n} seed {seed} M={M} counts {c2.tolist()}  <E> {ev2[0].item():.6f}")
    return M


def test_one_call_step_on_a_converged_network():
    """anchor(6) on LiH, 10^4 draws: M <= 4 unique samples.  naqs_vmc_step with m_lo = 1 equals the sampler +
    train_forward_eloc + train_backward_vmc + naqs_adam_step + set_weights bit for bit (the comparison of
    test_fused_step_calls_equal_their_parts); with m_lo = 10 it abandons the step and touches nothing.  At B = 6 the other
    physical keys hold 2.5e-9 of the mass (the 10^12-draw test's counts): that draw has M = 1, E_loc - <E> = 0 and a step that
    must move nothing.  A step that moves something, with 2 <= M <= 4: anchor(3) and 3 000 draws (1.2 draws off the anchor
    expected), the first of a hundred seeds whose draw has that many unique samples."""
    ham = _ham("LiH")
    cap = 1000
    assert _one_call_against_parts(ham, 10 ** 4, 77, cap) == 1
    fused, n = _step_net(3)[2], 3000
    seed = next((s_ for s_ in range(78, 178) if 2 <= len(fused.sample(n, s_, cap)[0]) <= 4), None)
    assert seed is not None, "no draw of 3 000 with 2..4 unique samples in a hundred seeds"
    assert 2 <= _one_call_against_parts(ham, n, seed, cap, B=3) <= 4
