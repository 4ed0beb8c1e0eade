"""Training on exact local energies on the MI355X: ``naqs_exact_eloc`` against the three library calls that define it, its
overflow contract, and the optimiser's exact step (``PartialSamplingOptimizer(..., exact_local_energies=True)``,
``-train_exact_eloc``) against the ordinary step where nothing is un-sampled, against float64, against its own pieces called
one by one, through a run to convergence, and on a network on the announced fallback.

The definition (include/naqs_hip.h):
    naqs_ham_connected(ham, M, keys, row_begin, n_rows, capacity, keys + M, &count)
    naqs_net_logpsi(net, count, keys + M, logpsi + M)
    naqs_eloc_reduced(ham, M + count, keys, logpsi, NAQS_LOGPSI_F32, row_begin, n_rows, w, eloc, out4)
"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import pytest

import grad_reference as gr
from conftest import GOLDEN, PKG
from test_eloc_gpu import all_keys, env  # noqa: F401 (env: fixture)
from test_exact_eloc import connected_reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TAU, GRAD_BOUND = 1e-5, 2e-5
EPS = 2.0 ** -53

FAMILIES = {
    "single": dict(aggregate=False),
    "aggregate": dict(aggregate=True, phase_hidden=(64,)),
    "single_L2": dict(aggregate=False, amp_layers=2),
    "aggregate_L2": dict(aggregate=True, amp_layers=2, phase_hidden=(64, 64)),
    "combined": dict(aggregate=False, combined=True),
}


def _net(mol, family="single", seed=3):
    """A default-initialised network on the molecule's sector in one of the handle families (grad_reference.sector_net's
    recipe; H2O and N2 have no entry in its SECTORS)."""
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    from test_nade import ELECTRONS
    f = dict(aggregate=False, amp_layers=1, phase_hidden=(512, 512), combined=False)
    f.update(FAMILIES[family])
    if mol in ELECTRONS:
        N, na, nb = ELECTRONS[mol]
    else:
        _, N, na, nb, _ = gr.sector(mol)
    hil = Hilbert.get(N, na, nb, encoding=Encoding.SIGNED, make_basis=N <= 14)
    torch.manual_seed(seed)
    wf = NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, amp_hidden_size=[64] * f["amp_layers"],
                                   phase_hidden_size=list(f["phase_hidden"]), use_amp_spin_sym=True, use_phase_spin_sym=False,
                                   aggregate_phase=f["aggregate"], combined_amp_phase_blocks=f["combined"],
                                   n_alpha_electrons=na, n_beta_electrons=nb)
    assert wf.fused(need_phase=True) is not None, (mol, family)
    return hil, wf


def _opt(mol, wf, tmp, **kw):
    from naqs_amd import packing
    from naqs_amd.optimizer import PartialSamplingOptimizer
    from test_nade import ELECTRONS
    from test_optimizer import ADAM
    N, na, nb = ELECTRONS[mol]
    ham = packing.load_packed(os.path.join(GOLDEN, f"ham_{mol}.npz"))
    args = dict(n_samples=100000, n_samples_max=1e12, n_unq_samples_min=10, n_unq_samples_max=1e5, log_exact_energy=False,
                wavefunction=wf, qubit_hamiltonian=ham, pre_compute_H=False, n_electrons=na + nb, n_alpha_electrons=na,
                n_beta_electrons=nb, normalise_psi=True, grad_clip_factor=None, optimizer=torch.optim.Adam,
                optimizer_args=[dict(a) for a in ADAM], save_loc=str(tmp), pauli_hamiltonian_dtype=np.float64, seed=5)
    args.update(kw)
    return PartialSamplingOptimizer(**args)


def _kdev(keys):
    return torch.as_tensor(np.asarray(keys, np.uint64).astype(np.int64), device="cuda")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _buffers(keys, lp, capacity, fill=None):
    M = keys.shape[0]
    kbuf = torch.zeros(M + capacity, dtype=torch.int64, device="cuda")
    lbuf = torch.full((M + capacity, 2), float("nan") if fill is None else fill, dtype=torch.float32, device="cuda")
    kbuf[:M] = keys
    lbuf[:M] = lp
    return kbuf, lbuf


def _three_calls(lib, fused, ham, keys, lp, b, n, capacity, w):
    """The definition, call by call -> (keys buffer, log-psi buffer, count, eloc, out4)."""
    from naqs_amd import _lib
    M = keys.shape[0]
    kbuf, lbuf = _buffers(keys, lp, capacity)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = lib.naqs_ham_connected(ham._h, M, kbuf.data_ptr(), b, n, capacity, (kbuf.data_ptr() + 8 * M) if capacity > 0 else None,
                                count.data_ptr(), _stream())
    _lib.check(st, "naqs_ham_connected")
    c = int(count.item())
    assert c <= capacity
    if c:
        _lib.check(lib.naqs_net_logpsi(fused._h, c, kbuf.data_ptr() + 8 * M, lbuf.data_ptr() + 8 * M, _stream()), "naqs_net_logpsi")
    eloc = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    out4 = torch.empty(4, dtype=torch.float64, device="cuda")
    st = lib.naqs_eloc_reduced(ham._h, M + c, kbuf.data_ptr(), lbuf.data_ptr(), _lib.LOGPSI_F32, b, n, w.data_ptr(), eloc.data_ptr(),
                               out4.data_ptr(), _stream())
    _lib.check(st, "naqs_eloc_reduced")
    torch.cuda.synchronize()
    return kbuf, lbuf, c, eloc, out4


def _check_call(lib, fused, ham, packed, table, b, n, rs):
    """One (table, row range): the call against its definition, the appended set against ``connected_reference``, the
    appended log psi against ``fused.log_psi``.  -> count."""
    keys = _kdev(table)
    M = keys.shape[0]
    lp = fused.log_psi(keys)
    w = torch.as_tensor(rs.random_sample(n) + 0.1, device="cuda")
    capacity = ham.connected_capacity(M, n)
    _, _, c_ref, e_ref, s_ref = _three_calls(lib, fused, ham, keys, lp, b, n, capacity, w)
    kbuf, lbuf = _buffers(keys, lp, capacity)
    e, s, count, overflow = fused.exact_local_energy(ham, kbuf, lbuf, M, b, n, capacity, weights=w)
    torch.cuda.synchronize()
    assert not overflow and count == c_ref, (M, b, n, count, c_ref)
    assert torch.equal(e, e_ref) and torch.equal(s, s_ref), (M, b, n)
    assert torch.equal(kbuf[:M], keys) and torch.equal(lbuf[:M], lp)                 # the table is an input and stays
    want = connected_reference(packed.xy, packed.n_qubits, packed.n_alpha, packed.n_beta, np.asarray(table, np.uint64), b, n)
    got = np.sort(kbuf[M:M + count].cpu().numpy().view(np.uint64))
    assert count == len(want) and np.array_equal(got, want), (M, b, n)
    if count:
        assert torch.equal(lbuf[M:M + count], fused.log_psi(kbuf[M:M + count].contiguous()))
    assert bool(torch.isnan(lbuf[M + count:]).all())                                  # nothing past the set
    # without weights: the same rows, no sums
    kbuf2, lbuf2 = _buffers(keys, lp, capacity)
    e2, s2, c2, _ = fused.exact_local_energy(ham, kbuf2, lbuf2, M, b, n, capacity)
    assert s2 is None and c2 == count and torch.equal(e2, e_ref)
    return count


def _ranges(M):
    b3 = min(3, M - 1)
    return sorted({(0, M), (b3, min(5, M - b3)), (M - 1, 1)})


# --------------------------------------------------------------------------------------------- 1. the call is its definition
@pytest.mark.parametrize("mol,family", [("LiH", f) for f in FAMILIES] + [("H2O", "single")])
def test_call_equals_its_three_call_definition(env, mol, family):
    packed = env["P"].load_packed(os.path.join(GOLDEN, f"ham_{mol}.npz"))
    ham = env["H"].DevicePauliHamiltonian(packed)
    hil, wf = _net(mol, family)
    fused = wf.fused(need_phase=True)
    space = all_keys(packed.n_qubits, packed.n_alpha, packed.n_beta)
    rs = np.random.RandomState(5)
    tables = [rs.permutation(space)[:M] for M in (1, 7, 64, 65)] + [space[::2], space]
    for table in tables:
        for b, n in _ranges(len(table)):
            count = _check_call(env["lib"].load_library(), fused, ham, packed, table, b, n, rs)
            if len(table) == len(space):
                assert count == 0                                # the whole sector: nothing is appended
            elif (b, n) == (0, len(table)):
                assert count > 0


def test_call_on_h2_the_smallest_sector(env):
    """P = 2: four states, tables of 1..4."""
    from test_pairs_gpu import _packed
    packed = _packed("H2")[0]
    ham = env["H"].DevicePauliHamiltonian(packed)
    hil, wf = gr.sector_net("H2", seed=3)
    fused = wf.fused(need_phase=True)
    assert fused is not None
    space = all_keys(4, 1, 1)
    rs = np.random.RandomState(6)
    for M in (1, 2, 3, 4):
        table = rs.permutation(space)[:M]
        for b, n in _ranges(M):
            _check_call(env["lib"].load_library(), fused, ham, packed, table, b, n, rs)


def test_call_on_n2_with_more_than_one_probe_and_drain_pass(env):
    packed = env["P"].load_packed(os.path.join(GOLDEN, "ham_N2.npz"))
    ham = env["H"].DevicePauliHamiltonian(packed)
    hil, wf = _net("N2")
    fused = wf.fused(need_phase=True)
    rs = np.random.RandomState(7)
    table = rs.permutation(all_keys(20, 7, 7))[:1000]
    for b, n in ((0, 1000), (3, 5)):
        count = _check_call(env["lib"].load_library(), fused, ham, packed, table, b, n, rs)
        assert count > (1000 if n == 1000 else 0)


def test_call_with_bit_31_set_in_table_and_set_keys(env):
    from test_pairs_gpu import _synthetic_32
    hil, wf = gr.sector_net("syn32_8_8", seed=3)
    fused = wf.fused(need_phase=True)
    assert fused is not None
    pool = gr.random_keys(hil, 4000, seed=23)
    pool = pool[(pool >> np.uint64(31)) & np.uint64(1) == 1]
    assert len(pool) > 200
    packed = _synthetic_32(pool)
    ham = env["H"].DevicePauliHamiltonian(packed)
    assert ham.key_bits == 32
    rs = np.random.RandomState(8)
    table = rs.permutation(pool)[:64]
    kset = []
    for b, n in _ranges(64):
        count = _check_call(env["lib"].load_library(), fused, ham, packed, table, b, n, rs)
        kset.append(count)
    want = connected_reference(packed.xy, 32, 8, 8, table, 0, 64)
    assert kset[0] == len(want) > 0 and np.all(want >> np.uint64(31) == 1) and np.all(table >> np.uint64(31) == 1)


# -------------------------------------------------------------------------------------------------------------- 2. overflow
def _half_table(mol, env):
    packed = env["P"].load_packed(os.path.join(GOLDEN, f"ham_{mol}.npz"))
    space = all_keys(packed.n_qubits, packed.n_alpha, packed.n_beta)
    return packed, space, space[::2]


def test_overflow_leaves_every_output_untouched(env):
    packed, space, table = _half_table("LiH", env)
    ham = env["H"].DevicePauliHamiltonian(packed)
    hil, wf = _net("LiH")
    fused = wf.fused(need_phase=True)
    keys = _kdev(table)
    M = keys.shape[0]
    lp = fused.log_psi(keys)
    w = torch.full((M,), 1.0 / M, dtype=torch.float64, device="cuda")
    full = len(connected_reference(packed.xy, packed.n_qubits, packed.n_alpha, packed.n_beta, table))
    assert full > 1
    for capacity in (full - 1, 0):
        kbuf, lbuf = _buffers(keys, lp, full)
        e = torch.full((M, 2), float("nan"), dtype=torch.float64, device="cuda")
        s = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
        _, _, count, overflow = fused.exact_local_energy(ham, kbuf, lbuf, M, 0, M, capacity, weights=w, out=e, sums_out=s)
        torch.cuda.synchronize()
        assert overflow and count > capacity, (capacity, count)
        assert bool(torch.isnan(e).all()) and bool(torch.isnan(s).all()) and bool(torch.isnan(lbuf[M:]).all())
        assert torch.equal(kbuf[:M], keys) and torch.equal(lbuf[:M], lp)
    kbuf, lbuf = _buffers(keys, lp, full)
    e, s, count, overflow = fused.exact_local_energy(ham, kbuf, lbuf, M, 0, M, full, weights=w)
    torch.cuda.synchronize()
    assert not overflow and count == full and bool(torch.isfinite(e).all()) and bool(torch.isfinite(s).all())


@pytest.mark.parametrize("mol", ["LiH", "H2O"])
def test_block_walk_rows_are_the_single_blocks_bits_and_sums_its_rounding(env, mol, tmp_path):
    """The optimiser's walk with the block length forced to 1, 7 and M / 2, and with a table limit that makes the first
    blocks overflow and halve: every ROW's bits are the single block's (``torch.equal``).
    A deliberate departure from "bit for bit" for the four weighted SUMS: the issue also asks that per-block sums be added
    in block order, and a sum of per-block reductions cannot have the bits of one in-kernel reduction over all rows.  They
    are held to the rounding of that other summation order instead, M eps sum_i |term_i| in float64 (M terms, each partial
    sum at most sum |term|): a bound from the number format, not from what the code gives."""
    packed, space, table = _half_table(mol, env)
    hil, wf = _net(mol)
    opt = _opt(mol, wf, tmp_path, exact_local_energies=True)
    fused = wf.fused(need_phase=True)
    keys = _kdev(table)
    M = keys.shape[0]
    rs = np.random.RandomState(3)
    w = torch.as_tensor(rs.random_sample(M) + 0.1, device="cuda")
    w = w / w.sum()

    def walk(first=None, max_table=2 ** 22):
        opt._exact_block_rows, opt.exact_max_table = first, max_table
        kbuf, lbuf = opt._exact_buffers(M)
        kbuf[:M].copy_(keys)
        fused.forward_saved(kbuf[:M], out=lbuf[:M])
        calls = []
        orig = fused.exact_local_energy
        fused.exact_local_energy = lambda *a, **k: (lambda r: (calls.append((a[4], a[5], r[3])), r)[1])(orig(*a, **k))
        try:
            e, s, n_conn = opt._exact_train_local_energy(fused, kbuf, lbuf, M, w)
        finally:
            del fused.exact_local_energy
        torch.cuda.synchronize()
        return e, s, n_conn, calls, opt._exact_block_rows

    e1, s1, n1, calls, kept = walk()
    assert calls == [(0, M, False)] and kept is None and n1 > 0
    terms = torch.stack([w * e1[:, 0], w * e1[:, 1], w * e1[:, 0] ** 2, w]).abs().sum(1)
    for first in (1, 7, M // 2):
        e, s, n_conn, calls, kept = walk(first)
        assert [c[:2] for c in calls] == [(b, min(first, M - b)) for b in range(0, M, first)] and not any(c[2] for c in calls)
        assert kept == first and n_conn >= n1
        assert torch.equal(e, e1)
        d = (s - s1).abs()
        print(f"[exact_train] {mol} blocks of {first}: sums off the single block's by {d.tolist()} (bound {(M * EPS * terms).tolist()})")
        assert bool((d <= M * EPS * terms).all())
    # halving: every row fits on its own, the whole table's set does not
    worst_row = max(len(connected_reference(packed.xy, packed.n_qubits, packed.n_alpha, packed.n_beta, table, r, 1)) for r in range(M))
    room = max(n1 // 3, worst_row)
    e, s, n_conn, calls, kept = walk(None, M + room)
    assert calls[0] == (0, M, True) and sum(n for _, n, over in calls if not over) == M and kept is not None and kept < M
    assert torch.equal(e, e1) and bool(((s - s1).abs() <= M * EPS * terms).all())
    # the next step starts from the length that fitted: no overflow is probed again
    e, s, n_conn, calls2, _ = walk(kept, M + room)
    assert not any(over for _, _, over in calls2) and torch.equal(e, e1)
    # a single row that does not fit is an error that names the row
    from naqs_amd._lib import NaqsError
    with pytest.raises(NaqsError, match=r"row \d+: more than 0 connected states outside the table of %d \(at least [1-9]" % M):
        walk(None, M)


# ------------------------------------------------------------------------------------------------------- 3. the whole space
@pytest.mark.parametrize("mol,family", [("LiH", "single"), ("H2O", "aggregate")])
def test_exact_step_on_the_whole_space_is_the_ordinary_step(env, mol, family, tmp_path):
    """Nothing is un-sampled: the connected set is empty, and the two steps give the same <E>, Var and parameters."""
    res = {}
    for exact in (True, False):
        hil, wf = _net(mol, family)
        opt = _opt(mol, wf, tmp_path / str(exact), exact_local_energies=exact)
        keys = _kdev(all_keys(hil.N, hil.N_alpha, hil.N_beta))
        lp = wf.fused(need_phase=True).log_psi(keys).double()
        w = (2.0 * lp[:, 0]).exp()
        w = (w / w.sum()).contiguous()
        E, var = opt._SGD_step(None, keys, None, sample_weights=w)
        res[exact] = (E, var, wf.flatten_parameters().clone(), opt._n_connected_pending)
    a, b = res[True], res[False]
    print(f"[exact_train] {mol} {family} whole space: <E> {a[0]!r} / {b[0]!r}, Var {a[1]!r} / {b[1]!r}")
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2])
    assert a[3] == 0 and np.isfinite(a[0])


# ------------------------------------------------------------------------------------------------ 4. gradient against float64
@pytest.mark.parametrize("mol", ["LiH", "H2O"])
def test_exact_step_gradient_against_float64(env, mol, tmp_path, capsys):
    """Half the sector sampled.  Reference, all float64: E_loc of the table's rows from the evaluation over the WHOLE space
    (where nothing is un-sampled) with log psi of the float64 copy of the network, the loss gradient of those, and the float64
    network's parameter gradient.  Rows within TAU of a ReLU kink carry no weight (tests/test_agg_depth_gpu.py's rule)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    hil, wf = _net(mol)
    opt = _opt(mol, wf, tmp_path, exact_local_energies=True)
    ham = opt.pauli_hamiltonian
    space = all_keys(hil.N, hil.N_alpha, hil.N_beta)
    pos = np.arange(0, len(space), 2)
    kd = _kdev(space)
    _, w64 = gr.f64_copy(wf)
    states = hil.idx2state(kd).cpu()
    lp_full = gr.log_psi_f64(w64, states)
    e_full = ham.local_energy(kd, torch.as_tensor(lp_full, device="cuda"), kind="log_psi").cpu().numpy()
    e_loc = e_full[pos]
    st = states[pos]
    lp64, margin = gr.log_psi_and_kink_margin(w64, st)
    w = np.exp(2.0 * lp_full[pos, 0])
    w[margin < TAU] = 0.0
    w /= w.sum()
    g, dropped = gr.kink_free(gr.loss_grad_f64(e_loc, w), margin, TAU)
    want = gr.grad_f64(w64, st, g, lp=lp64)
    want_abs = gr.grad_f64(w64, st, np.abs(g))
    keys, wd = kd[torch.as_tensor(pos, device="cuda")].contiguous(), torch.as_tensor(w, device="cuda")
    ref = opt.evaluate_energy(keys=keys, weights=wd, exact=True)
    trunc = opt.evaluate_energy(keys=keys, weights=wd, exact=False)
    grads = {}
    step = opt.optimizer.step

    def grab(*a, **k):
        grads.update({n: p.grad.detach().double().cpu().numpy().copy() for n, p in wf.model.named_parameters()})
        return step(*a, **k)

    opt.optimizer.step = grab
    E, var = opt._SGD_step(None, keys, None, sample_weights=wd)
    worst = 0.0
    for name in want:
        scale = max(np.abs(want[name]).max(), 0.1 * np.abs(want_abs[name]).max())
        err = np.abs(grads[name] - want[name]).max() / scale if scale > 0 else np.abs(grads[name]).max()
        worst = max(worst, err)
    d_e, d_v = abs(E - ref["E"]) / abs(ref["E"]), abs(var - ref["Var"]) / abs(ref["Var"])
    with capsys.disabled():
        print(f"\n[exact_train] {mol} half table ({len(pos)} rows, {dropped} at a kink, {opt._n_connected_pending} connected): "
              f"gradient worst {worst:.2e} of the tensor scale; <E> {E:.10f} (evaluate_energy: rel {d_e:.1e}), Var {var:.6f} "
              f"(rel {d_v:.1e}); truncated <E> {trunc['E']:.10f}, differs by {abs(trunc['E'] - E):.3e} Ha")
    assert opt._n_connected_pending == ref["n_connected"] > 0
    assert d_e <= 1e-12 and d_v <= 1e-12, (d_e, d_v)
    assert abs(trunc["E"] - E) > 1e-6
    for name in want:
        scale = max(np.abs(want[name]).max(), 0.1 * np.abs(want_abs[name]).max())
        err = np.abs(grads[name] - want[name]).max() / scale if scale > 0 else np.abs(grads[name]).max()
        assert err <= GRAD_BOUND, (mol, name, err)


# ------------------------------------------------------------------------------------------------------------ 5. composition
@pytest.mark.parametrize("mol,family", [("LiH", "single"), ("LiH", "aggregate"), ("H2O", "single")])
def test_exact_step_is_its_pieces_called_one_by_one(env, mol, family, tmp_path):
    from naqs_amd.flat_adam import FlatAdam
    packed, space, table = _half_table(mol, env)
    keys = _kdev(table)
    M = keys.shape[0]
    w = torch.as_tensor(np.random.RandomState(4).random_sample(M) + 0.1, device="cuda")
    w = (w / w.sum()).contiguous()
    # the step
    hil, wf = _net(mol, family)
    opt = _opt(mol, wf, tmp_path / "step", exact_local_energies=True)
    E, var = opt._SGD_step(None, keys, None, sample_weights=w)
    # the pieces
    hil2, wf2 = _net(mol, family)
    opt2 = _opt(mol, wf2, tmp_path / "pieces", exact_local_energies=True)
    assert isinstance(opt2.optimizer, FlatAdam)
    fused, ham = wf2.fused(need_phase=True), opt2.pauli_hamiltonian
    capacity = ham.connected_capacity(M, M)
    kbuf = torch.empty(M + capacity, dtype=torch.int64, device="cuda")
    lbuf = torch.empty((M + capacity, 2), dtype=torch.float32, device="cuda")
    kbuf[:M] = keys
    lp, saved = fused.forward_saved(kbuf[:M], out=lbuf[:M])
    e, s, count, overflow = fused.exact_local_energy(ham, kbuf, lbuf, M, 0, M, capacity, weights=w)
    assert not overflow and count > 0
    g, ev = fused.vmc_loss_grad(e, w, s, with_energy=True)
    opt2.optimizer.zero_grad()
    fused.backward_saved(saved, g)
    opt2.optimizer.step()
    wf2.parameters_changed()
    E2, var2 = ev.tolist()
    assert (E, var) == (E2, var2)
    assert torch.equal(wf.flatten_parameters(), wf2.flatten_parameters())
    assert opt._n_connected_pending == count


def test_exact_run_is_the_hand_loop_and_fuses_nothing(env, tmp_path, capsys, monkeypatch):
    from naqs_amd.optimizer import LogKey
    lib = env["lib"].load_library()
    res = {}
    for how in ("run", "hand"):
        hil, wf = _net("LiH")
        opt = _opt("LiH", wf, tmp_path / how, exact_local_energies=True, n_samples=2000)
        fused = wf.fused(need_phase=True)
        assert not opt._can_prefuse() and not opt._can_onecall()

        def refuse(*a, **k):
            raise AssertionError("a fused sampler call in exact mode")

        for name in ("sample_forward_local_energy", "vmc_step", "vmc_run", "forward_saved_with_local_energy"):
            monkeypatch.setattr(fused, name, refuse)
        monkeypatch.setattr(wf, "sample_with_local_energy", refuse)
        launches0 = lib.naqs_launch_count()
        if how == "run":
            opt.run(n_epochs=20, save_freq=None, save_final=False, output_freq=10)
            e = np.array([x[1] for x in opt.log[LogKey.E_LOC]])
            v = np.array([x[1] for x in opt.log[LogKey.E_LOC_VAR]])
            assert [s for s, _ in opt.n_connected] == [1, 10, 20] and all(n > 0 for _, n in opt.n_connected)
        else:
            ev = []
            opt._in_run = True
            opt._choose_dist_mode()
            for _ in range(20):
                states, counts, probs = opt.get_samples(lazy=True)
                assert opt._prefused is None
                ev.append(opt._SGD_step(states, opt._sample_keys, None, sample_weights=opt._sample_weights, lazy=True))
                opt.n_steps += 1
            opt._in_run = False
            ev = torch.stack(ev).cpu().numpy()
            e, v = ev[:, 0], ev[:, 1]
        torch.cuda.synchronize()
        res[how] = (e, v, wf.flatten_parameters().clone(), lib.naqs_launch_count() - launches0)
    capsys.readouterr()
    a, b = res["run"], res["hand"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and torch.equal(a[2], b[2])
    # run() adds nothing to the hand loop but its output lines (calculate_energy is off: log_exact_energy=False)
    assert a[3] == b[3], (a[3], b[3])
    assert np.isfinite(a[0]).all() and a[0][-1] < a[0][0]


# ------------------------------------------------------------------------------------------------------------------ 6. a run
FLAGS = ["-single_phase", "-n1", "-n_layer", "1", "-n_hid", "64", "-n_layer_phase", "2", "-n_hid_phase", "512",
         "-n_train", "10000", "-output_freq", "1000", "-save_freq", "-1"]


def test_training_to_convergence_on_exact_local_energies(tmp_path, capsys):
    """tests/test_config3_gpu.py's run and criteria with -train_exact_eloc; the truncated run beside it for the variance."""
    sys.path.insert(0, PKG)
    import pandas as pd
    from experiments import _base
    from naqs_amd.optimizer import LogKey
    kat = json.load(open(os.path.join(GOLDEN, "kat.json")))
    fci = kat["fci"]["H2O"]
    out = {}
    for tag, extra in (("exact", ["-train_exact_eloc"]), ("truncated", [])):
        t0 = time.time()
        res = _base.run(molecule=None, out=None, number=1, lr=-1, n_samps=1e7, n_samps_max=1e12, n_unq_samps_min=1e4,
                        n_unq_samps_max=1e5, n_hid=128, n_layer=1, reweight_samples_by_psi=False, n_train=10000, n_pretrain=0,
                        output_freq=25, save_freq=-1, load_hamiltonian=False, overwrite_hamiltonian=False,
                        presolve_hamiltonian=False, cont=False, n_excitations_max=-1, use_amp_spin_sym=True,
                        use_phase_spin_sym=False, comb_amp_phase=False, aggregate_phase=True, restrict_H=True, reset_opt=False,
                        argv=["-m", os.path.join(GOLDEN, "ham_H2O.npz"), "-o", str(tmp_path / tag), "-s", "111"] + FLAGS + extra)
        wall = time.time() - t0
        text = capsys.readouterr().out
        log = pd.read_pickle(tmp_path / tag / "log.pkl")
        out[tag] = (res[0], wall, text, float(log[LogKey.E_LOC_VAR].iloc[-1]), float(log[LogKey.E_LOC_VAR].iloc[-50:].mean()))
    r, wall, text, var, var50 = out["exact"]
    rt, wall_t, _, var_t, var50_t = out["truncated"]
    with capsys.disabled():
        print(f"\n[exact_train] H2O 10 000 steps: exact final <E_loc> {r['final']:.8f} Ha, subspace {r['eig']:.8f} Ha, FCI {fci:.8f} Ha, "
              f"final Var {var:.3e} (mean of last 50 {var50:.3e}), training {r['time']:.1f} s (wall {wall:.1f} s); truncated final "
              f"{rt['final']:.8f} Ha, Var {var_t:.3e} ({var50_t:.3e}), training {rt['time']:.1f} s (wall {wall_t:.1f} s)")
    assert "run as PyTorch modules" not in text                       # no fallback notice: the HIP kernels throughout
    assert "\ttrain_exact_eloc : True" in text
    assert -1e-5 < r["final"] - fci < 1e-3, (r["final"], fci)
    assert -1e-8 < r["eig"] - fci < 1e-4, (r["eig"], fci)
    summary = open(tmp_path / "exact" / "summary.txt").read()
    assert "trained on : exact local energies (psi on every connected state)" in summary
    assert "trained on : truncated local energies" in open(tmp_path / "truncated" / "summary.txt").read()


# -------------------------------------------------------------------------------------------------------- 7. fallback network
def test_exact_steps_of_a_network_on_the_fallback(env, tmp_path, capsys):
    """LiH_combampphase's shape (-comb_amp_phase with the aggregate phase): PyTorch modules and autograd, the Python evaluator."""
    from test_exact_eloc_gpu import _net as eloc_net
    hil, wf = eloc_net("LiH", fallback=True)
    assert wf.fused() is None
    opt = _opt("LiH", wf, tmp_path, exact_local_energies=True, n_samples=300)
    before = torch.cat([p.detach().reshape(-1) for p in wf.model.parameters()]).clone()
    for _ in range(3):
        states, counts, probs = opt.get_samples()
        keys, w = opt._sample_keys, opt._sample_weights
        assert keys.shape[0] < hil.size                        # something IS un-sampled
        ref = opt.evaluate_energy(keys=keys, weights=w, exact=True)
        E, var = opt._SGD_step(states, keys, None, sample_weights=w)
        opt.n_steps += 1
        assert abs(E - ref["E"]) <= 1e-9 * max(1.0, abs(ref["E"])), (E, ref["E"])
        assert ref["n_connected"] > 0 and np.isfinite(var)
    after = torch.cat([p.detach().reshape(-1) for p in wf.model.parameters()])
    assert float((after - before).abs().max()) > 0
    assert opt._n_connected_pending > 0
    capsys.readouterr()
