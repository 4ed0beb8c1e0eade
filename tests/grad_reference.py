"""The float64 reference of the training backward (a plain helper module, like oracle_backend.py).

The PyTorch formulation of the network (naqs_amd.nade) follows the dtype of its parameters, so a float64 copy of a network
on the CPU is an exact-arithmetic stand-in for what the HIP backward computes in float32:

* ``f64_copy``                 the same network, on the CPU, in float64 (or any other dtype);
* ``log_psi_and_kink_margin``  log psi plus, per row, the smallest |input| of any ReLU — rows whose margin is within
                               rounding of zero may take the other branch in float32 (a different, equally valid gradient);
* ``grad_f64``                 d/d theta sum_i g_i . log psi_i per parameter name;
* ``loss_grad_f64`` / ``loss_grad_f32_emulated``
                               d loss / d (log|psi|, phase) of the VMC loss of _SGD_step (energy.py:328-329): exactly, and in
                               the float32 arithmetic vmc_grad_kernel documents (naqs_grad.hip);
* ``kink_free``                g with the rows near a kink zeroed;
* ``log_psi_f64``              the forward alone, in chunks of rows (no graph): float64 numpy [M, 2];
* ``sorted_rows``              the first m rows of a key set in the library's (ascending) order, with their reference rows;
* ``log_amp_f64``              log|psi| alone, from the amplitude blocks' conditionals (no phase MLP): the sampler's target;
* ``conditionals_f64``         one block's four conditional probabilities for a set of prefixes (the sampler's tree nodes);
* ``SECTORS`` / ``sector_net`` one electron sector per orbital-pair count P = 2..16 and a default-initialised network on it;
* ``random_keys``              distinct random physical keys of any sector;
* ``anchor`` / ``rebalance`` / ``outlier_unit`` / ``grown``
                               recipes that take a default-initialised network to the regime of a trained one: |psi|^2
                               peaked on one determinant, weights of unequal magnitude within a block, a unit that sets
                               a block's maxima and never fires, grown weights;
* ``tree_levels`` / ``tree_chi2``
                               the sampling tree of one draw and its level-by-level multinomial test;
* ``pair_ordering`` / ``relabel_keys`` / ``model_index``
                               qubit orderings other than -1: a seeded spin-preserving pair permutation as a
                               ``qubit2model`` list, the same model-order bits under another ordering, and the rank of a
                               key in the sampler's (prefix, outcome) order.
"""
import contextlib

import numpy as np
import torch
from torch import nn

from conftest import golden


def f64_copy(src, dtype=torch.float64):
    """``src``: a ``nade_<fixture>.npz`` name (``"N2_aggphase"``) or a ``NAQSComplex_NADE_orbitals`` on any device ->
    (hilbert, the same network on the CPU in ``dtype``)."""
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    if isinstance(src, str):
        from test_nade import make_wf
        from test_variants import split
        try:
            mol = split(src)[0]
        except ValueError:                  # a base fixture: nade_<mol>.npz
            mol = src
        hil, wf = make_wf(mol, golden(f"nade_{src}.npz"))
    else:
        m = src.model
        lin = m.phase_layers[0].linears() if len(m.phase_layers) else []
        wf = NAQSComplex_NADE_orbitals(
            src.hilbert, qubit_ordering=[int(q) for q in src.qubit2model_permutation], masking=m.masking,
            amp_hidden_size=[l.out_features for l in m.amp_layers[0].linears()[:-1]],
            phase_hidden_size=[l.out_features for l in lin[:-1]], use_amp_spin_sym=m.use_amp_spin_sym,
            use_phase_spin_sym=m.use_phase_spin_sym, aggregate_phase=m.aggregate_phase,
            combined_amp_phase_blocks=m.combined_amp_phase_blocks,
            n_alpha_electrons=m.n_alpha_up if m.use_restricted_hilbert else None,
            n_beta_electrons=m.n_beta_up if m.use_restricted_hilbert else None, device="cpu")
        wf.model.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
        hil = src.hilbert
    wf.model.to(dtype)
    return hil, wf


@contextlib.contextmanager
def _relu_inputs(model, sink):
    """Record min |x| over each row of every ReLU input while the block is active: forward pre-hooks on the nn.ReLU modules
    (the single phase MLP) and a wrapper around torch.relu (the amplitude blocks and the per-pair phase blocks, nade.py)."""
    def note(x):
        sink.append(x.detach().abs().reshape(x.shape[0], -1).amin(1))

    hooks = [mod.register_forward_pre_hook(lambda mod, args: note(args[0])) for mod in model.modules()
             if isinstance(mod, nn.ReLU)]
    relu = torch.relu

    def wrapped(x, *a, **k):
        note(x)
        return relu(x, *a, **k)

    torch.relu = wrapped
    try:
        yield
    finally:
        torch.relu = relu
        for h in hooks:
            h.remove()


def log_psi_and_kink_margin(wf, states):
    """states: [M, N] (+-1, qubit order) -> (log psi [M, 2] with its autograd graph, margin float64 numpy [M]: the smallest
    |pre-activation| of any ReLU the row passes through)."""
    mins = []
    with _relu_inputs(wf.model, mins):
        lp = wf.log_psi(states).reshape(-1, 2)
    M = lp.shape[0]
    margin = torch.full((M,), float("inf"), dtype=torch.float64)
    for m in mins:
        margin = torch.minimum(margin, m.double())
    return lp, margin.numpy()


def grad_f64(wf, states, g, lp=None):
    """{parameter name: d/d theta sum_i g[i] . log psi_i} as float64 numpy arrays (float64 network: exact to ~1e-15); ``lp``:
    a log psi of these states with its graph, when the caller already has one."""
    if lp is None:
        lp = wf.log_psi(states).reshape(-1, 2)
    names, params = zip(*wf.model.named_parameters())
    g = torch.as_tensor(np.asarray(g), dtype=lp.dtype).reshape(-1, 2)
    grads = torch.autograd.grad((lp * g).sum(), params, allow_unused=True)
    return {n: (np.zeros(tuple(p.shape)) if d is None else d.double().numpy()) for n, p, d in zip(names, params, grads)}


def loss_grad_f64(eloc, w):
    """d loss / d (log|psi|, phase) of loss = 2 Re sum_i w_i log psi_i (E_i - <E>)^*, <E> = sum_i w_i E_i (energy.py:328-329),
    in float64.  eloc: complex [M] or float [M, 2]; w: [M] -> [M, 2]."""
    e = _complex(eloc)
    w = np.asarray(w, np.float64)
    d = e - (w * e).sum()
    return np.stack([2 * w * d.real, -2 * w * d.imag], -1)


def loss_grad_f32_emulated(eloc, w, sums):
    """vmc_grad_kernel's arithmetic (naqs_grad.hip): g = (((float)Re E - (float)sums[0]) * (2 (float)w),
    -(((float)Im E - (float)sums[1]) * (2 (float)w))), every operation rounded to float32."""
    e = _complex(eloc)
    f = np.float32
    two_w = f(2.0) * np.asarray(w, np.float64).astype(f)
    m_re, m_im = f(sums[0]), f(sums[1])
    return np.stack([(e.real.astype(f) - m_re) * two_w, -((e.imag.astype(f) - m_im) * two_w)], -1)


def kink_free(g, margin, tau=1e-5):
    """g with the rows whose margin is below tau zeroed -> (g, number of rows zeroed)."""
    g = np.array(g, copy=True)
    near = np.asarray(margin) < tau
    g[near] = 0
    return g, int(near.sum())


def _complex(eloc):
    e = np.asarray(eloc)
    if np.iscomplexobj(e):
        return e.astype(np.complex128)
    return e[..., 0].astype(np.float64) + 1j * e[..., 1].astype(np.float64)


def log_psi_f64(wf, states, chunk=4096):
    """log psi [M, 2] of ``states`` ([M, N] +-1, qubit order) through the network ``wf`` (an ``f64_copy``: float64, or float32
    for the CPU float32 error it is compared with), as float64 numpy.  The forward is row-independent: chunks of rows give
    the same numbers as one pass and bound the memory of the [512, 512] networks."""
    states = torch.as_tensor(states)
    out = np.empty((states.shape[0], 2), np.float64)
    with torch.no_grad():
        for lo in range(0, states.shape[0], chunk):
            out[lo:lo + chunk] = wf.log_psi(states[lo:lo + chunk]).reshape(-1, 2).double().numpy()
    return out


def sorted_rows(keys, m, *tables):
    """keys: the key set a reference was computed on, in its own order; -> (its first m keys ascending — the order the
    library's tables are kept in —, then each table's rows in that order)."""
    order = np.argsort(keys[:m], kind="stable")
    return (keys[:m][order],) + tuple(t[:m][order] for t in tables)


def _model_order(wf, states):
    """[M, N] (+-1, qubit order) -> (alpha, beta) occupations [M, P] (+-1) per model pair, in the network's dtype."""
    dt = next(wf.model.parameters()).dtype
    x = torch.as_tensor(states)[..., wf._q2m.cpu()].to(dt)
    return x[:, 0::2], x[:, 1::2]


def conditionals_f64(wf, states, n):
    """Block n's conditionals for the prefixes of ``states`` ([U, N] +-1, qubit order; only model pairs 0..n-1 are read):
    -> (p float64 [U, 4] = exp(2 log-amplitude) per outcome (a, b) -> a + 2 b, physical mask bool [U, 4]).  With the
    softmax masked (FULL, or PARTIAL before the last pair) p sums to one over the physical outcomes and is 0 elsewhere."""
    a, b = _model_order(wf, states)
    with torch.no_grad():
        la, phys = wf.model._block_log_amp(n, a[:, :n], b[:, :n])
    return torch.exp(2 * la).double().numpy(), phys.numpy()


def log_amp_f64(wf, states, chunk=1 << 16):
    """log|psi| [M] of ``states`` ([M, N] +-1, qubit order) as the sum over pairs of the chosen outcome's conditional
    log-amplitude (OrbitalNADE._block_log_amp, the sampler's formulation): log_psi_f64(...)[:, 0] without the phase MLP."""
    states = torch.as_tensor(states)
    out = np.empty(states.shape[0], np.float64)
    with torch.no_grad():
        for lo in range(0, states.shape[0], chunk):
            a, b = _model_order(wf, states[lo:lo + chunk])
            occ = ((a > 0).long() + 2 * (b > 0).long())
            acc = torch.zeros(a.shape[0], dtype=torch.float64)
            for n in range(wf.model.P):
                la, _ = wf.model._block_log_amp(n, a[:, :n], b[:, :n])
                acc += la.gather(1, occ[:, n:n + 1]).squeeze(1).double()
            out[lo:lo + chunk] = acc.numpy()
    return out


# One sector per orbital-pair count P = 2..16: (name, qubits, n_alpha, n_beta, molecule of packing_terms.npz or None for a
# synthetic sector).  P = 10 adds the extreme fillings: 1 of 10 alpha orbitals (H2_cc-pvdz), 9 of 10 (F2), 9 / 7 (O2).
SECTORS = [
    ("H2", 4, 1, 1, "H2"),
    ("syn6_2_1", 6, 2, 1, None),              # synthetic, open shell
    ("H2_6-31G", 8, 1, 1, "H2_6-31G"),
    ("syn10_3_2", 10, 3, 2, None),            # synthetic: the one level after the sampler's head
    ("LiH", 12, 2, 2, "LiH"),
    ("BeH2", 14, 3, 3, "BeH2"),
    ("NH3", 16, 5, 5, "NH3"),
    ("CH4", 18, 5, 5, "CH4"),
    ("LiF", 20, 6, 6, "LiF"),
    ("H2_cc-pvdz", 20, 1, 1, "H2_cc-pvdz"),
    ("F2", 20, 9, 9, "F2"),
    ("O2", 20, 9, 7, "O2"),
    ("H2S", 22, 9, 9, "H2S"),
    ("PH3", 24, 9, 9, "PH3"),
    ("H2O_6-31G", 26, 5, 5, "H2O_6-31G"),
    ("LiCl", 28, 10, 10, "LiCl"),
    ("Li2O", 30, 7, 7, "Li2O"),
    ("syn32_8_8", 32, 8, 8, None),            # synthetic: the ABI's 16 pairs, 32-bit keys
]


def sector(name):
    return next(r for r in SECTORS if r[0] == name)


def sector_net(name, device="cuda", seed=0, masking="PARTIAL", aggregate=False, phase_sym=False, amp_layers=1, amp_hidden=64,
               phase_hidden=(512, 512), combined=False, qubit_ordering=-1):
    """(hilbert, network) on sector ``name``: default-initialised from ``seed``; by default the published shape (amplitude
    width 64, one phase MLP [512, 512], amplitude spin symmetry, PARTIAL masking).  ``aggregate``: one phase block of
    ``phase_hidden`` per pair (run.py's default ansatz); ``amp_layers``: hidden layers per amplitude block; ``combined``: -comb_amp_phase (the
    last block's output layer carries the phase rows); ``qubit_ordering``: -1, +1 or a ``qubit2model`` list (the weights
    drawn from ``seed`` do not depend on it)."""
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.nade import NadeMasking
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    _, N, na, nb, _ = sector(name)
    hil = Hilbert.get(N, na, nb, encoding=Encoding.SIGNED)
    torch.manual_seed(seed)
    wf = NAQSComplex_NADE_orbitals(hil, device=device, qubit_ordering=qubit_ordering, masking=NadeMasking[masking],
                                   amp_hidden_size=[amp_hidden] * amp_layers, phase_hidden_size=list(phase_hidden),
                                   use_amp_spin_sym=True, use_phase_spin_sym=phase_sym, aggregate_phase=aggregate,
                                   combined_amp_phase_blocks=combined, n_alpha_electrons=na, n_beta_electrons=nb)
    return hil, wf


def random_keys(hil, M, seed):
    """M distinct physical keys of ``hil``'s sector (even qubits alpha, odd beta), in random order; M <= hil.size."""
    assert M <= hil.size, (M, hil.size)
    rs = np.random.RandomState(seed)
    N, na, nb = hil.N, hil.N_alpha, hil.N_beta
    keys = np.zeros(0, np.uint64)
    while len(keys) < M:
        a = np.argsort(rs.random_sample((2 * M, N // 2)), 1)
        ka = (np.uint64(1) << (2 * a[:, :na]).astype(np.uint64)).sum(1, dtype=np.uint64)
        b = np.argsort(rs.random_sample((2 * M, N // 2)), 1)
        kb = (np.uint64(1) << (2 * b[:, :nb] + 1).astype(np.uint64)).sum(1, dtype=np.uint64)
        keys = np.unique(np.concatenate([keys, ka | kb]))
    return rs.permutation(keys)[:M]


# ------------------------------------------------------------------------------------------------- peaked networks
def _anchor_occ(wf):
    """Per model pair the anchor's outcome (0 empty, 1 alpha only, 3 both) and the amplitude output that feeds it alone:
    the last n_beta pairs doubly occupied (output 2), n_alpha - n_beta pairs before them singly (output 1), the rest empty
    (output 0).  Outputs 0 and 2 enter one outcome each with or without the spin symmetrisation; output 1 feeds |10> (and,
    symmetrised, |01>)."""
    m = wf.model
    assert m.use_restricted_hilbert and m.use_amp_spin_sym and m.n_alpha_up >= m.n_beta_up
    P, na, nb = m.P, m.n_alpha_up, m.n_beta_up
    return [0] * (P - na) + [1] * (na - nb) + [3] * nb, [0] * (P - na) + [1] * (na - nb) + [2] * nb


def anchor(wf, B, open_shell=False):
    """Add the bias ``B`` to the amplitude output of every block that feeds the anchor determinant's outcome: |psi|^2 peaks on
    that determinant (one softmax logit 2 B above the others per pair) -> the anchor key (uint64, qubit order of the
    network's qubit_ordering).  Closed-shell sectors unless ``open_shell``: there the n_alpha - n_beta singly occupied
    pairs get the bias on output 1, shared by |10> and |01>, and the key returned is the alpha one."""
    m = wf.model
    assert open_shell or m.n_alpha_up == m.n_beta_up, "anchor: a closed-shell sector (open_shell=True for the other form)"
    occ, outs = _anchor_occ(wf)
    q2m = [int(q) for q in wf.qubit2model_permutation]
    key = 0
    with torch.no_grad():
        for n, (o, j) in enumerate(zip(occ, outs)):
            m.amp_layers[n].linears()[-1].bias[j] += B
            if o & 1:
                key |= 1 << q2m[2 * n]
            if o & 2:
                key |= 1 << q2m[2 * n + 1]
    return np.uint64(key)


def _parts(wf, part):
    """``part`` -> the lists of (lower Linear, upper Linear) it names: ("amp", n[, l]) hidden layer l of amplitude block n;
    ("phase", l) hidden layer l of every phase block (the single MLP, or each aggregate block)."""
    m = wf.model
    if part[0] == "amp":
        lin = m.amp_layers[part[1]].linears()
        l = part[2] if len(part) > 2 else 0
        return [(lin[l], lin[l + 1])]
    assert part[0] == "phase"
    return [(blk.linears()[part[1]], blk.linears()[part[1] + 1]) for blk in m.phase_layers]


def rebalance(wf, k, part):
    """relu(2^k x) = 2^k relu(x): W_l, b_l of ``part`` times 2^k and W_{l+1} times 2^-k (b_{l+1} untouched) is the same
    function, and — a power of two commutes with every float32 rounding short of under- and overflow — the same float32
    bits.  -> (names of the parameters multiplied by 2^k, names multiplied by 2^-k): their gradients are the original's
    times 2^-k and 2^k."""
    names = {id(p): n for n, p in wf.model.named_parameters()}
    up, down = [], []
    with torch.no_grad():
        for lo, hi in _parts(wf, part):
            lo.weight.mul_(2.0 ** k)
            lo.bias.mul_(2.0 ** k)
            hi.weight.mul_(2.0 ** -k)
            up += [names[id(lo.weight)], names[id(lo.bias)]]
            down.append(names[id(hi.weight)])
    return up, down


def outlier_unit(wf, R):
    """Hidden unit 0 of every amplitude block's first layer: its W1 row times ``R`` and b1[0] = -2 R sum_k |W1[0][k]| (the
    inputs are +-1 or 0: the unit never fires), its W2 column unchanged.  The network is the same function; the unit sets
    the first layer's weight maximum and the largest pre-activation bound of the block.  -> names of the tensors it touched."""
    names = {id(p): n for n, p in wf.model.named_parameters()}
    out = []
    with torch.no_grad():
        for blk in wf.model.amp_layers:
            lin = blk.linears()[0]
            lin.bias[0] = -2.0 * R * lin.weight[0].abs().sum()
            lin.weight[0].mul_(R)
            out += [names[id(lin.weight)], names[id(lin.bias)]]
    return out


def grown(wf, out_factor=4.0, hidden_factor=2.0, B=6.0):
    """Every block's output layer (weights and bias) times ``out_factor``, every hidden layer times ``hidden_factor``, then
    ``anchor(B)``: weights that have left U(+-1/sqrt(fan_in)) -> the anchor key."""
    with torch.no_grad():
        for blk in list(wf.model.amp_layers) + list(wf.model.phase_layers):
            lin = blk.linears()
            for l, layer in enumerate(lin):
                f = out_factor if l == len(lin) - 1 else hidden_factor
                layer.weight.mul_(f)
                layer.bias.mul_(f)
    return anchor(wf, B)


# ------------------------------------------------------------------------------------ the sampling tree of one draw
def tree_levels(wf64, hil, k, c):
    """The sampling tree of one draw (keys ``k``, counts ``c``): per level, each node's children counts [U, 4], float64
    conditionals [U, 4] and physical mask [U, 4]."""
    st = hil.idx2state(torch.as_tensor(np.asarray(k).astype(np.int64)))
    ms = st[:, wf64._q2m.cpu()]
    occ = ((ms[:, 0::2] > 0).long() + 2 * (ms[:, 1::2] > 0).long()).numpy().astype(np.int64)
    code = np.zeros(len(k), np.int64)
    levels = []
    for n in range(occ.shape[1]):
        _, first, inv = np.unique(code, return_index=True, return_inverse=True)
        cc = np.zeros((len(first), 4))
        np.add.at(cc, (inv.reshape(-1), occ[:, n]), c)
        levels.append((cc,) + conditionals_f64(wf64, st[first], n))
        code = code + occ[:, n] * (4 ** n)
    return levels


def tree_chi2(levels, root=None, replace=None, min_lump=0.0):
    """Level-by-level test: every node's count splits into children counts ~ Multinomial(count, p), p the node's float64
    conditionals; cells of >= 5 expected draws, the rest of a node pooled; a node left with one cell is skipped.
    -> (pooled chi2, dof, p-value, per-level p-values, draws of masked children, per-level share of the draws in skipped
    nodes that have two or more physical children [a node whose electron budget leaves one child has nothing to test]).
    ``root``: the root's p replaced; ``replace``: (level, node, p) one node's p replaced.  ``min_lump``: a pooled cell
    expecting fewer draws than this joins the node's smallest cell of >= 5 (on a peaked tree a node of 10^5 draws has
    children expecting 10^-3: one draw there is a chi-square term of 10^3 the chi-square law does not describe).
    For FULL masking, which drops no draw (nade.py:695)."""
    from scipy import stats
    tot, dof, per_level, masked_hits, skipped = 0.0, 0, [], 0, []
    for n, (cc, pc, phys) in enumerate(levels):
        if n == 0 and root is not None:
            pc = root[None, :]
        if replace is not None and replace[0] == n:
            pc = pc.copy()
            pc[replace[1]] = replace[2]
        masked_hits += int(cc[pc == 0].sum())
        e = cc.sum(1, keepdims=True) * pc
        node_draws = cc.sum(1)
        big = e >= 5
        chi = np.where(big, (cc - e) ** 2 / np.where(big, e, 1), 0).sum(1)
        so, se = np.where(big, 0, cc).sum(1), np.where(big, 0, e).sum(1)
        if min_lump > 0:
            join = (se > 0) & (se < min_lump) & big.any(1)
            j = np.where(big, e, np.inf).argmin(1)
            rows = np.flatnonzero(join)
            cc, e = cc.copy(), e.copy()
            cc[rows, j[rows]] += so[rows]
            e[rows, j[rows]] += se[rows]
            so, se = np.where(join, 0, so), np.where(join, 0, se)
            chi = np.where(big, (cc - e) ** 2 / np.where(big, e, 1), 0).sum(1)
        lump = se > 0
        chi += np.where(lump, (so - se) ** 2 / np.where(lump, se, 1), 0)
        cells = big.sum(1) + lump
        keep = cells >= 2
        lv_chi, lv_dof = chi[keep].sum(), int((cells[keep] - 1).sum())
        per_level.append(stats.chi2.sf(lv_chi, lv_dof) if lv_dof else 1.0)
        skipped.append(node_draws[~keep & (phys.sum(1) >= 2)].sum() / max(node_draws.sum(), 1))
        tot += lv_chi
        dof += lv_dof
    return tot, dof, stats.chi2.sf(tot, dof) if dof else 1.0, per_level, masked_hits, skipped


def pair_ordering(P, seed):
    """A ``qubit2model`` list [2 p, 2 p + 1 for p in pi] of a seeded permutation pi of the P orbital pairs: spin preserving
    (alpha stays on even model positions), and neither the identity (ordering +1) nor the reversal (ordering -1)."""
    assert P >= 3, "two pairs have no permutation besides the identity and the reversal"
    rs = np.random.RandomState(seed)
    while True:
        pi = rs.permutation(P)
        if not (np.array_equal(pi, np.arange(P)) or np.array_equal(pi, np.arange(P)[::-1])):
            break
    assert sorted(pi.tolist()) == list(range(P))
    assert pi.tolist() != list(range(P)) and pi.tolist() != list(range(P))[::-1]
    return [int(q) for p in pi for q in (2 * p, 2 * p + 1)]


def q2m_of(ordering, N):
    """The ``qubit2model`` list of ordering -1 / +1 (wavefunction.py:78-85), or the list itself."""
    if isinstance(ordering, int):
        assert ordering in (1, -1)
        return list(range(N)) if ordering == 1 else [q for p in range(N // 2 - 1, -1, -1) for q in (2 * p, 2 * p + 1)]
    return [int(q) for q in ordering]


def relabel_keys(keys, q2m_from, q2m_to):
    """Bit ``q2m_from[i]`` of each input key becomes bit ``q2m_to[i]`` of the output (uint64 [M]): the key that shows a
    network at ordering ``q2m_to`` the model-order occupations the input shows one at ``q2m_from``."""
    keys = np.asarray(keys).astype(np.uint64)
    assert len(q2m_from) == len(q2m_to)
    out = np.zeros_like(keys)
    for f, t in zip(q2m_from, q2m_to):
        out |= ((keys >> np.uint64(f)) & np.uint64(1)) << np.uint64(t)
    return out


def model_index(keys, q2m):
    """sum_n occ_n 4^(P-1-n) with occ_n = alpha + 2 beta of model pair n (int64 [M]; P <= 16 fits): the rank of a key in
    the (prefix, outcome) order the sampler emits its table in."""
    keys = np.asarray(keys).astype(np.uint64)
    P = len(q2m) // 2
    idx = np.zeros(keys.shape, np.int64)
    for n in range(P):
        a = ((keys >> np.uint64(q2m[2 * n])) & np.uint64(1)).astype(np.int64)
        b = ((keys >> np.uint64(q2m[2 * n + 1])) & np.uint64(1)).astype(np.int64)
        idx = idx * 4 + a + 2 * b
    return idx
