"""The float64 reference of the natural-gradient step (a plain helper module, like grad_reference.py).

Definitions (include/naqs_hip.h, naqs_net_sr_gram): log psi_i = a_i + i phi_i, A = d a / d theta, B = d phi / d theta
(M x N_p, columns in state_dict order), weights w (sum 1), D = diag(sqrt w), seeds g [M, 2]:

    X_a = D (A - 1 w^T A),   T_a = X_a X_a^T,   y_a = g[:, 0] / (2 sqrt w)          (X_phi, T_phi, y_phi from B, g[:, 1])
    lambda = diag_shift * mean(diag T)                                              (per block)
    d theta = X_a^T (T_a + lambda I)^-1 y_a + X_phi^T (T_phi + lambda I)^-1 y_phi

* ``CASES`` / ``make_net`` / ``table``   the networks and key tables tests/test_sr_gpu.py runs, one sector each;
* ``jacobians``                          A, B row by row through torch.autograd.grad on a CPU copy of the network (float64: the
                                         reference; float32: the yardstick, its rows taken to float64 before any product);
* ``gram_err``                           max_ij |G - G64|_ij / sqrt(G64_ii G64_jj);
* ``system`` / ``direction``             the definitions above in float64 numpy (dense solve);
* ``direction_f32``                      the same step as a float32 network on the CPU takes it: the direction's yardstick;
* ``LARGE_CASES`` / ``sampled_rows`` / ``rows_below`` / ``seeds_f64`` / ``WIDTH_CASES``
                                         tables of up to 4 300 rows (tests/test_sr_scale_gpu.py): G_ij depends on rows i and j
                                         alone, so the float64 Jacobian rows of ~80 sampled rows check G[R][:, R] at any M; the
                                         centring is ``centred`` of the device's own G; X^T x is one float64 backward with seeds.
* ``SHAPE_CASES`` / ``SYM_CASES`` / ``ORDER_CASES`` / ``shape_net`` / ``shape_id`` / ``SEEDS``
                                         every phase width and depth class, -phase_sym in both families and orderings other than
                                         -1 (tests/test_sr_shapes.py, tests/test_sr_shapes_gpu.py), tables of at most 130 rows.
"""
import numpy as np
import torch

import grad_reference as gr

TAU = 1e-5          # kink margin (float64 pre-activation) below which a row is left out, as in the backward tests

# (sector, aggregate, amp_hidden, phase_hidden, amp_sym, masking).  Not the full product of the axes — each value of every axis
# (family x amplitude width x phase shape x symmetry x masking) meets each sector at least once where the sector allows it, and
# each pair of values of two axes meets somewhere:  H2 (P = 2: pair 0's constant input is half the network), syn10_3_2 (P = 5: one
# level behind the sampler's head), LiH (P = 6), syn32_8_8 (P = 16: the ABI's largest, bit 31 of the keys in use).
CASES = [
    ("H2", False, 16, (32,), True, "PARTIAL"),
    ("H2", True, 16, (32,), False, "FULL"),
    ("syn10_3_2", False, 64, (64, 64), True, "FULL"),
    ("syn10_3_2", True, 64, (32,), True, "PARTIAL"),
    ("LiH", False, 16, (32,), False, "PARTIAL"),
    ("LiH", False, 64, (64, 64), True, "PARTIAL"),
    ("LiH", True, 16, (32,), True, "FULL"),
    ("syn32_8_8", False, 64, (32,), True, "PARTIAL"),
    ("syn32_8_8", False, 16, (64, 64), False, "FULL"),
    ("syn32_8_8", True, 64, (32,), False, "PARTIAL"),
]
ROWS = (1, 63, 64, 65, 200)     # the tile edge, padded rows, I = J and I < J tiles; capped by the sector's size (H2: 4, syn10_3_2: 100)


# The same step at the table sizes a run on N2 has (tests/test_sr_scale_gpu.py).  LiF single: 44 100 states and N_p = 3 206 < M, T is
# rank-deficient and the shift carries the factorisation; LiF aggregate: Ha = 128 amplitude blocks (8 waves), P = 10; syn32_8_8:
# P = 16 (32 jobs = SR_MAX_JOBS), bit 31 of the keys, grad_in_kernel in the phase chain.
LARGE_CASES = [
    ("LiF", False, 16, (32,), True, "PARTIAL"),
    ("LiF", True, 128, (32,), True, "PARTIAL"),
    ("syn32_8_8", False, 64, (64, 64), True, "PARTIAL"),
]
LARGE_ROWS = 4300                                           # 67 full 64-row tiles and one of 12 rows
LARGE_SIZES = (1023, 1024, 1025, 4095, 4096, 4097, 4300)    # the scratch's first capacity (1 024), the tile loop's second trip (64 x 64)
FIXED_ROWS = (0, 63, 64, 255, 256, 257, 1022, 1023, 1024, 1025, 4094, 4095, 4096, 4097, 4299)

# amplitude widths beside 16 and 64: 2, 3, 6 and 8 waves per workgroup of sr_amp_factors_kernel; kh = 32, 64, 96, 128 of ldh = 64, 64,
# 128, 128 columns (48, like 16, leaves padding columns inside the products' reach)
WIDTH_CASES = [("LiH", agg, ha, (32,), True, "PARTIAL") for agg in (False, True) for ha in (32, 48, 96, 128)]
WIDTH_ROWS = (65, 200)


# ---- every phase shape the natural-gradient entries accept (tests/test_sr_shapes.py, tests/test_sr_shapes_gpu.py) ----
# (sector, aggregate, amp_hidden, phase_hidden, PHASE_sym, masking): the amplitude symmetry is on throughout (``shape_net`` builds
# on grad_reference.sector_net).  sr_gram_kernel reads kd = pad32(N) columns of a layer's deltas and ka = pad32(K) of its inputs
# out of the training scratch, whose leading dimensions are pad64; sr_jvp_kernel deals (layer, 64 columns) items to at most 16
# workgroups per tile.  Each shape is named for the branch it reaches.
_SHAPES = [
    ((1,), "one chunk, 31 padding columns read"),
    ((5,), "one chunk, 27 padding columns read"),
    ((33,), "two chunks, the second 31 padding columns"),
    ((48,), "two chunks, 16 padding columns read of leading dimension 64"),
    ((17, 17), "hidden to hidden with padding: kd and ka both 32 for 17"),
    ((100, 200), "128 and 224 columns read from leading dimensions 128 and 256"),
    ((96, 96), "a multiple of 32, not of 64: leading dimension 128, 96 columns read"),
    ((160, 32), "leading dimension 192, 160 columns read"),
    ((496, 496), "512 columns read, 16 of them padding; 17 JVP items: the deal wraps"),
    ((512, 512), "the published shape; 17 JVP items"),
    ((512, 512, 512), "25 JVP items, depth 3"),
    ((16,) * 8, "9 jobs through phase_src_off"),
    ((64,) * 8, "9 jobs, no padding"),
]
SHAPE_CASES = [("LiH", False, 16, ph, False, "PARTIAL") for ph, _ in _SHAPES] + [
    ("H2", False, 16, (48,), False, "PARTIAL"),                  # 2 phase inputs, 4 states
    ("H2", False, 16, (512, 512), False, "PARTIAL"),
    ("syn32_8_8", False, 16, (48,), False, "PARTIAL"),           # 30 phase inputs, bit 31 of the keys
    ("syn32_8_8", False, 16, (512, 512), False, "PARTIAL"),
    ("LiH", False, 64, (512, 512), False, "PARTIAL"),            # the published network
]
SYM_CASES = [
    ("LiH", False, 16, (16, 16), True, "PARTIAL"),
    ("LiH", False, 16, (48,), True, "PARTIAL"),
    ("LiH", False, 16, (112,), True, "PARTIAL"),
    ("LiH", False, 16, (512, 512), True, "PARTIAL"),
    ("syn10_3_2", False, 16, (48,), True, "PARTIAL"),            # open shell: the abits > bbits swap is not symmetric
    ("LiH", True, 16, (32,), True, "PARTIAL"),
    ("syn10_3_2", True, 16, (32,), True, "FULL"),
    ("LiH", True, 64, (48,), True, "FULL"),
    ("syn10_3_2", True, 64, (48,), True, "PARTIAL"),
]
# (index into CASES, ordering: +1 or "pi" = grad_reference.pair_ordering(P, ORDER_SEED)): LiH single [64, 64], LiH aggregate,
# syn32_8_8 single — held to float64 at -1 by tests/test_sr_gpu.py, here bit for bit against that handle
ORDER_CASES = [(i, o) for i in (5, 6, 7) for o in (1, "pi")]
ORDER_SEED = 4
SHAPE_ROWS = (1, 65, 130)       # one row, I = J with padded rows, I < J tiles; capped by the sector (H2: 4, syn10_3_2: 100)
SHAPE_TABLE = max(SHAPE_ROWS)
SHAPE_SEED = 3                  # make_net's default
SEEDS = {}                      # shape_id -> seed where SHAPE_SEED leaves fewer than ``rows_wanted`` kink-free rows


def shape_id(case):
    name, agg, ha, ph, psym, mask = case
    shape = "x".join(map(str, ph)) if len(set(ph)) > 1 or len(ph) < 3 else f"{ph[0]}_x{len(ph)}"
    return f"{name}-{'agg' if agg else 'single'}-a{ha}-p{shape}-{'psym' if psym else 'nopsym'}-{mask}"


def shape_net(case, device="cuda", qubit_ordering=-1):
    """(hilbert, network) of a SHAPE_CASES / SYM_CASES entry, default-initialised from its seed."""
    name, agg, ha, ph, psym, mask = case
    return gr.sector_net(name, device=device, seed=SEEDS.get(shape_id(case), SHAPE_SEED), masking=mask, aggregate=agg, phase_sym=psym,
                         amp_hidden=ha, phase_hidden=ph, qubit_ordering=qubit_ordering)


def rows_wanted(hil):
    """min(130, the sector less a tenth): what a case's kink-free table must hold."""
    return min(SHAPE_TABLE, int(np.ceil(0.9 * hil.size)))


def shape_rows(n):
    return sorted({min(m, n) for m in SHAPE_ROWS})


def order_of(o, P):
    return o if o == 1 else gr.pair_ordering(P, ORDER_SEED)


def split_jacobian(A, B):
    """No parameter moves both log|psi| and the phase: (A + B, the columns that are B's) holds both in half the memory."""
    pcols = (B != 0).any(0)
    assert not np.any(pcols & (A != 0).any(0))
    A += B
    return A, pcols


def sampled_rows(n=LARGE_ROWS, extra=64, seed=11):
    """R_all: FIXED_ROWS and ``extra`` seeded random rows of a table of ``n`` rows, ascending."""
    rs = np.random.RandomState(seed)
    return np.unique(np.concatenate([np.asarray(FIXED_ROWS), rs.choice(n, extra, replace=False)]))


def rows_below(R_all, M):
    """The sampled rows of the leading M rows together with the last row M - 1 (FIXED_ROWS holds it for every size of
    LARGE_SIZES) -> (rows, their positions in R_all)."""
    rows = np.unique(np.concatenate([R_all[R_all < M], [M - 1]]))
    pos = np.searchsorted(R_all, rows)
    assert np.array_equal(R_all[pos], rows), M
    return rows, pos


def seeds_f64(w, x):
    """s_i = sqrt(w_i) x_i - w_i sum_j sqrt(w_j) x_j in float64: X^T x is the backward pass with these seeds."""
    sw = np.sqrt(w)
    return sw * x - w * (sw @ x)


def flat(wf, grads):
    """A {name: array} of per-parameter arrays -> one float64 vector in state_dict order."""
    return np.concatenate([np.asarray(grads[n], np.float64).reshape(-1) for n, _ in wf.model.named_parameters()])


def case_id(case):
    name, agg, ha, ph, sym, mask = case
    return f"{name}-{'agg' if agg else 'single'}-a{ha}-p{'x'.join(map(str, ph))}-{'sym' if sym else 'nosym'}-{mask}"


def make_net(case, device="cuda", seed=3, qubit_ordering=-1):
    """(hilbert, network) of a case, default-initialised from ``seed`` (the parameters are drawn on the CPU: the same on any device
    and at any ``qubit_ordering``)."""
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.nade import NadeMasking
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    name, agg, ha, ph, sym, mask = case
    _, N, na, nb, _ = gr.sector(name)
    hil = Hilbert.get(N, na, nb, encoding=Encoding.SIGNED)
    torch.manual_seed(seed)
    wf = NAQSComplex_NADE_orbitals(hil, device=device, qubit_ordering=qubit_ordering, masking=NadeMasking[mask], amp_hidden_size=[ha],
                                   phase_hidden_size=list(ph), use_amp_spin_sym=sym, use_phase_spin_sym=False, aggregate_phase=agg,
                                   n_alpha_electrons=na, n_beta_electrons=nb)
    return hil, wf


def states_of(hil, keys):
    return hil.idx2state(torch.as_tensor(np.asarray(keys).astype(np.int64)))


def table(hil, w64, rows=max(ROWS), seed=5):
    """Up to ``rows`` distinct keys of the sector in ascending order, none within TAU of a ReLU kink of the float64 network, and
    random positive weights (sum 1 over the whole table; a leading part is renormalised by its user)."""
    cand = np.sort(gr.random_keys(hil, min(hil.size, rows + rows // 4), seed=seed))
    _, margin = gr.log_psi_and_kink_margin(w64, states_of(hil, cand))
    keys = cand[margin >= TAU][:rows]
    rs = np.random.RandomState(seed + 1)
    w = rs.random_sample(len(keys)) + 0.1
    return keys, w / w.sum()


def jacobians(wf, states):
    """(A, B) float64 numpy [M, N_p]: rows d log|psi_i| / d theta and d phase_i / d theta of the CPU network ``wf`` in its own
    dtype, one torch.autograd.grad per row and component, columns in state_dict order."""
    params = list(wf.model.parameters())
    lp = wf.log_psi(states).reshape(-1, 2)
    M = lp.shape[0]
    out = np.zeros((2, M, sum(p.numel() for p in params)))
    for i in range(M):
        for c in range(2):
            gs = torch.autograd.grad(lp[i, c], params, retain_graph=True, allow_unused=True)
            out[c, i] = torch.cat([(torch.zeros_like(p) if g is None else g).reshape(-1) for p, g in zip(params, gs)]).double().numpy()
    return out[0], out[1]


def gram_err(G, G64):
    d = np.sqrt(np.diag(G64))
    scale = np.outer(d, d)
    return float(np.max(np.abs(np.asarray(G, np.float64) - G64) / np.where(scale > 0, scale, 1.0)))


def system(J, w, g_col, diag_shift):
    """One block: (T + lambda I, y, X) float64 from the Jacobian J [M, N_p], weights w [M] and a column of the seeds."""
    sw = np.sqrt(w)
    X = sw[:, None] * (J - (w @ J)[None, :])
    T = X @ X.T
    lam = diag_shift * np.trace(T) / len(w)
    return T + lam * np.eye(len(w)), np.asarray(g_col, np.float64) / (2 * sw), X


def centred(G, w, diag_shift):
    """T + lambda I from an uncentred Gram matrix: D (G - m 1^T - 1 m^T + c) D, m = G w, c = w^T G w."""
    sw = np.sqrt(w)
    m = G @ w
    T = sw[:, None] * (G - m[:, None] - m[None, :] + w @ m) * sw[None, :]
    return T + diag_shift * np.trace(T) / len(w) * np.eye(len(w))


def direction(A, B, w, g, diag_shift):
    """d theta float64 [N_p] by dense solves."""
    out = 0.0
    for J, col in ((A, 0), (B, 1)):
        T, y, X = system(J, w, np.asarray(g)[:, col], diag_shift)
        out = out + X.T @ np.linalg.solve(T, y)
    return out


def direction_f32(w32, states, A32, B32, w, g, diag_shift):
    """The float32-CPU pipeline, the yardstick of the kernels' direction: float32 Jacobian rows of the float32 network ``w32``, the
    two systems and their solves in float64, the seeds s_i = sqrt(w_i) x_i - w_i sum_j sqrt(w_j) x_j rounded to float32, and
    X^T x as the float32 autograd backward of sum_i s_i . log psi_i — what ``naqs_net_sr_direction`` does with its kernels."""
    sw = np.sqrt(w)
    seeds = []
    for J, col in ((A32, 0), (B32, 1)):
        T, y, _ = system(J, w, np.asarray(g)[:, col], diag_shift)
        x = np.linalg.solve(T, y)
        seeds.append(sw * x - w * (sw @ x))
    grads = gr.grad_f64(w32, states, np.stack(seeds, -1).astype(np.float32))
    return np.concatenate([grads[n].reshape(-1) for n, _ in w32.model.named_parameters()])


def per_tensor_err(wf, got, want):
    """max over the parameter tensors of max |got - want| / max |want| on the tensor's slice of the flat vectors (the backward
    tests' measure; a tensor whose reference slice is zero — pair 0's first-layer weights see a constant-zero input — must be zero)."""
    return per_tensor_worst(wf, got, want)[0]


def per_tensor_worst(wf, got, want):
    """``per_tensor_err`` and the name of the tensor that sets it."""
    worst, who, off = 0.0, None, 0
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    for name, p in wf.model.named_parameters():
        n = p.numel()
        a, b = got[off:off + n], want[off:off + n]
        off += n
        scale = np.abs(b).max()
        if scale == 0:
            assert np.all(a == 0), name
            continue
        err = float(np.abs(a - b).max() / scale)
        if err > worst or who is None:
            worst, who = err, name
    return worst, who
