"""Exact local energies on the MI355X: psi evaluated on the connected states the sample table does not hold.

``naqs_ham_connected`` (connected_kernel) against the numpy restatement of its definition (tests/test_exact_eloc.py), its
capacity contract, and ``calculate_local_energy(set_unsampled_states_to_zero=False)`` / ``evaluate_energy`` / ``-exact_eloc``
on top of it: against the existing E_loc kernel and the oracle over the WHOLE restricted space (where nothing is unsampled),
at an eigenstate (zero variance, which the truncated mode cannot give), and with psi from the networks.

Measured on an MI355X: the set equal in every case; against the E_loc kernel over the whole space 0 (bit-identical), against
the oracle <= 8.1e-15; at the FCI vector the exact rows within 1.2e-11 (LiH) / 7.9e-10 Ha (H2O) of E0 and the truncated rows off
by 25.7 / 158 Ha; the network cases at 0.000 of their float64-derived bound (test_exact_mode_with_psi_from_the_network).
"""
import json
import os
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, PKG, dense_pauli_case, golden
from test_eloc_gpu import all_keys, dev_ham, env, random_physical_keys, rel_err, run_eloc, synth_logpsi  # noqa: F401 (env: fixture)
from test_exact_eloc import connected_reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


# ----------------------------------------------------------------------------------------------------------- the set
def _packed(env, mol):
    return env["P"].load_packed(os.path.join(GOLDEN, f"ham_{mol}.npz"))


def _synthetic(env, N, na, nb, n_keys, seed, filtered=True, need_bit=None):
    """test_64bit_keys' construction: random physical keys, flip masks = xor of random key pairs (+ the diagonal), a few
    terms each.  -> (packed Hamiltonian, pool of keys).  ``need_bit``: keep only keys with that bit set."""
    rs = np.random.RandomState(seed)
    keys = random_physical_keys(N, na, nb, n_keys, seed)
    if need_bit is not None:
        keys = keys[(keys >> np.uint64(need_bit)) & np.uint64(1) == 1]
        assert len(keys) > 200
    pairs = rs.randint(0, len(keys), size=(300, 2))
    xys = np.unique(np.r_[np.uint64(0), keys[pairs[:, 0]] ^ keys[pairs[:, 1]]])
    xy = np.repeat(xys, rs.randint(1, 6, size=len(xys)))
    yz = rs.randint(0, 1 << 20, size=len(xy)).astype(np.uint64)
    cf = rs.normal(size=len(xy))
    perm = rs.permutation(len(xy))
    P = env["P"]
    return P.PackedHamiltonian(N, na if filtered else -1, nb if filtered else -1, xy[perm], yz[perm], cf[perm]), keys


def _case(env, name):
    """-> (packed Hamiltonian, pool of keys the tables are cut from, whether the pool is the whole sector)."""
    P = env["P"]
    if name in ("LiH", "H2O", "N2", "CH2"):
        p = _packed(env, name)
        return p, all_keys(p.n_qubits, p.n_alpha, p.n_beta), True
    lih = _packed(env, "LiH")
    space = all_keys(12, 2, 2)
    if name == "few_groups":                                   # fewer groups than a wave has lanes (the diagonal + 40)
        keep = np.isin(lih.xy, np.unique(lih.xy)[:41])
        return P.PackedHamiltonian(12, 2, 2, lih.xy[keep], lih.yz[keep], lih.coeff[keep]), space, True
    if name == "no_diagonal":
        nd = lih.xy != 0
        return P.PackedHamiltonian(12, 2, 2, lih.xy[nd], lih.yz[nd], lih.coeff[nd]), space, True
    if name == "K0":
        z = np.zeros(0, np.uint64)
        return P.PackedHamiltonian(12, 2, 2, z, z, np.zeros(0)), space, True
    if name == "unrestricted6":
        terms, _, _ = dense_pauli_case(6)
        return P.pack_qubit_hamiltonian(terms, 6, -1, -1), np.arange(64, dtype=np.uint64), True
    if name == "bit31":
        p, keys = _synthetic(env, 32, 3, 3, 4000, 23, need_bit=31)
        return p, keys, False
    if name in ("q40_filtered", "q40_unfiltered"):
        p, keys = _synthetic(env, 40, 6, 6, 1500, 17, filtered=name == "q40_filtered")
        return p, keys, False
    raise KeyError(name)


CASES = ["LiH", "H2O", "N2", "CH2", "few_groups", "no_diagonal", "K0", "unrestricted6", "bit31", "q40_filtered", "q40_unfiltered"]


def _connected(env, ham, keys, b=0, n=None, capacity=None):
    k = env["H"].keys_to_device(np.asarray(keys, np.uint64), ham.device)
    got, count = ham.connected_keys(k, row_begin=b, n_rows=n, capacity=capacity)
    return (None if got is None else got.cpu().numpy().view(np.uint64)), count


@pytest.mark.parametrize("name", CASES)
def test_connected_set_is_exactly_the_definition(env, name):
    p, pool, whole = _case(env, name)
    ham = env["H"].DevicePauliHamiltonian(p)
    assert ham.key_bits == (64 if p.n_qubits > 32 else 32)
    if name == "bit31":
        assert np.all(pool >> np.uint64(31) == 1)
    rs = np.random.RandomState(5)
    sizes = sorted({1, 7, 64, 65, len(pool) // 2, len(pool) - 1, len(pool)} & set(range(1, len(pool) + 1)))
    kernels = set()
    for M in sizes:
        keys = rs.permutation(pool)[:M]                          # unsorted, like a sampler's table
        for b, n in {(0, M), (min(3, M - 1), min(5, M - min(3, M - 1))), (M - 1, 1), (M // 2, 0)}:
            got, count = _connected(env, ham, keys, b, n)
            want = connected_reference(p.xy, p.n_qubits, p.n_alpha, p.n_beta, keys, b, n)
            assert count == len(want), (M, b, n, count, len(want))
            assert np.array_equal(got, want), (M, b, n)
            if n:
                kernels.add(ham.last_kernel())
        if whole and M == len(pool):
            assert _connected(env, ham, keys)[1] == 0            # nothing is outside the whole sector
    if name != "K0":
        assert kernels and all(k.startswith(f"connected_kernel<uint{ham.key_bits}_t") for k in kernels), kernels
    if name == "N2":
        assert any("NT=1024" in k for k in kernels) and any("NT=256" in k for k in kernels), kernels


def test_connected_set_has_no_repeats_where_many_rows_share_a_key(env):
    """N2, 2 000 random rows: ~16 candidates per key outside the table, found by waves of many workgroups."""
    p = _packed(env, "N2")
    ham = env["H"].DevicePauliHamiltonian(p)
    keys = np.random.RandomState(11).permutation(all_keys(20, 7, 7))[:2000]
    got, count = _connected(env, ham, keys)
    want = connected_reference(p.xy, 20, 7, 7, keys)
    uxy = np.unique(p.xy)
    cand = keys[:, None] ^ uxy[None, 1:]
    ok = (np.bitwise_count(cand & np.uint64(0x55555)) == 7) & (np.bitwise_count(cand & np.uint64(0xAAAAA)) == 7)
    n_cand = int((ok & ~np.isin(cand, keys)).sum())
    assert n_cand > 8 * len(want)                               # the duplication this case is about
    assert count == len(want) == len(np.unique(got)) and np.array_equal(got, want)
    # the Bloom form (the handle builds the filter when forced; 1024-thread workgroups)
    os.environ["NAQS_BLOOM"] = "1"
    try:
        got_b, _ = _connected(env, ham, keys)
        assert "BLOOM=1" in ham.last_kernel()
    finally:
        del os.environ["NAQS_BLOOM"]
    assert np.array_equal(got_b, want)


# ---------------------------------------------------------------------------------------------------------- capacity
@pytest.mark.parametrize("mol,M", [("LiH", 112), ("N2", 2000)])
def test_capacity_contract(env, mol, M):
    p = _packed(env, mol)
    ham = env["H"].DevicePauliHamiltonian(p)
    space = all_keys(p.n_qubits, p.n_alpha, p.n_beta)
    keys = np.random.RandomState(3).permutation(space)[:M]
    lp = synth_logpsi(M, 4)
    before = run_eloc(env, ham, keys, lp, kind="log_psi", dtype=torch.float64)
    want = connected_reference(p.xy, p.n_qubits, p.n_alpha, p.n_beta, keys)
    size = len(want)
    assert size > 64
    t0 = time.perf_counter()
    got, count = _connected(env, ham, keys, capacity=size)
    t_ok = time.perf_counter() - t0
    assert count == size and np.array_equal(got, want)
    for cap in (size - 1, size // 2, 1, 0):
        t0 = time.perf_counter()
        got, count = _connected(env, ham, keys, capacity=cap)
        dt = time.perf_counter() - t0
        assert got is None and count > cap, (cap, count)
        assert dt < 10 * t_ok + 1.0, (cap, dt, t_ok)            # an overflowing call is a count, not a wait
    got, count = _connected(env, ham, keys, capacity=size + 5)
    assert count == size and np.array_equal(got, want)
    after = run_eloc(env, ham, keys, lp, kind="log_psi", dtype=torch.float64)
    assert np.array_equal(before, after)                        # the handle's ordinary calls are untouched


# ------------------------------------------------------------------------------------------ E_loc, psi supplied everywhere
def _bare_optimizer(ham):
    """``calculate_local_energy`` without a network behind it: the exact mode with ``psi_fn`` reads the Hamiltonian, the
    device and two switches of the optimiser, nothing else."""
    from naqs_amd.optimizer import OptimizerBase
    opt = object.__new__(OptimizerBase)
    opt.pauli_hamiltonian, opt.device = ham, ham.device
    opt.bug_compat_full_sample_order, opt.use_fused, opt.wavefunction = False, False, None
    return opt


def _lookup(space, table, device):
    """psi_fn: a look-up into a float64 table over the whole (ascending) space."""
    sk = torch.as_tensor(space.astype(np.int64), device=device)
    tb = torch.as_tensor(table, dtype=torch.float64, device=device)

    def psi_fn(keys):
        pos = torch.searchsorted(sk, keys)
        assert torch.equal(sk[pos], keys)
        return tb[pos]
    return psi_fn


_FULL = {}


def _full_space(env, mol):
    """Per molecule, once: the space, synthetic (log|psi|, phase) on it, the existing kernel's E_loc and the oracle's over
    the whole space."""
    if mol not in _FULL:
        h = golden(f"ham_{mol}.npz")
        ham = dev_ham(env, mol)
        space = all_keys(int(h["n_qubits"]), int(h["n_alpha"]), int(h["n_beta"]))
        lp = synth_logpsi(len(space), 21)
        e_dev = run_eloc(env, ham, space, lp, kind="log_psi", dtype=torch.float64)
        psi = np.exp(lp[:, 0]) * np.exp(1j * lp[:, 1])
        e_orc = env["O"].eloc_matrix_free(h["xy"], h["yz"], h["coeff"], space, psi)
        _FULL[mol] = (ham, space, lp, e_dev, e_orc)
    return _FULL[mol]


def _complex(e):
    e = e.cpu().numpy()
    return e[:, 0] + 1j * e[:, 1]


@pytest.mark.parametrize("mol,sizes", [("LiH", (1, 7, 64, 65, 112, 224, 225)), ("H2O", (1, 7, 64, 65, 220, 440, 441)), ("N2", (1000,))])
def test_exact_mode_equals_the_whole_space_evaluation(env, mol, sizes):
    ham, space, lp, e_dev, e_orc = _full_space(env, mol)
    opt = _bare_optimizer(ham)
    psi_fn = _lookup(space, lp, ham.device)
    rs = np.random.RandomState(8)
    for M in sizes:
        pos = rs.permutation(len(space))[:M]
        keys = torch.as_tensor(space[pos].astype(np.int64), device=ham.device)
        e = _complex(opt.calculate_local_energy(keys, set_unsampled_states_to_zero=False, psi_fn=psi_fn))
        d_dev = np.max(np.abs(e - e_dev[pos]) / np.maximum(1.0, np.abs(e_dev[pos])))
        d_orc = rel_err(e, e_orc[pos])
        print(f"[exact_eloc] {mol} M={M}: vs the E_loc kernel over the whole space {d_dev:.2e}, vs the oracle {d_orc:.2e}")
        assert d_dev <= 1e-12, (M, d_dev)
        assert d_orc <= 1e-10, (M, d_orc)
        # (Re, Im) given for the sampled rows are used as they are; psi_fn serves the rest
        if M in (65, 1000):
            psi_s = torch.as_tensor(np.stack([np.exp(lp[pos, 0]) * np.cos(lp[pos, 1]), np.exp(lp[pos, 0]) * np.sin(lp[pos, 1])], -1),
                                    device=ham.device)
            e2 = _complex(opt.calculate_local_energy(keys, psi=psi_s, set_unsampled_states_to_zero=False, psi_fn=psi_fn))
            assert rel_err(e2, e_orc[pos]) <= 1e-10
            # a row range: the rows' own numbers
            e3 = _complex(opt.calculate_local_energy(keys, set_unsampled_states_to_zero=False, psi_fn=psi_fn, row_begin=3, n_rows=5))
            assert np.array_equal(e3, e[3:8])
    # the default mode is the truncated one, as before: it differs on a half table
    pos = rs.permutation(len(space))[:len(space) // 2]
    keys = torch.as_tensor(space[pos].astype(np.int64), device=ham.device)
    lp_s = torch.as_tensor(lp[pos], device=ham.device)
    trunc = _complex(opt.calculate_local_energy(keys, log_psi=lp_s))
    assert np.array_equal(trunc, run_eloc(env, ham, space[pos], lp[pos], kind="log_psi", dtype=torch.float64))
    assert rel_err(trunc, e_orc[pos]) > 1e-3


@pytest.mark.parametrize("mol,M", [("LiH", 112), ("H2O", 220), ("N2", 1000)])
def test_forced_block_splitting_changes_no_bit(env, mol, M):
    """A row's hit set and summation order do not depend on what else the table holds."""
    from naqs_amd._lib import NaqsError
    ham, space, lp, _, _ = _full_space(env, mol)
    opt = _bare_optimizer(ham)
    psi_fn = _lookup(space, lp, ham.device)
    pos = np.random.RandomState(9).permutation(len(space))[:M]
    keys = torch.as_tensor(space[pos].astype(np.int64), device=ham.device)
    whole = opt.calculate_local_energy(keys, set_unsampled_states_to_zero=False, psi_fn=psi_fn)
    h = golden(f"ham_{mol}.npz")
    na, nb, N = int(h["n_alpha"]), int(h["n_beta"]), int(h["n_qubits"])
    n_all = ham.connected_keys(keys)[1]
    worst_row = max(len(connected_reference(h["xy"], N, na, nb, space[pos], r, 1)) for r in range(M))
    room = max(n_all // 3, worst_row)                           # every row fits on its own, the whole table's set does not
    blocks = []
    orig = ham.local_energy
    ham.local_energy = lambda *a, **k: (blocks.append((k["row_begin"], k["n_rows"])), orig(*a, **k))[1]
    try:
        split = opt.calculate_local_energy(keys, set_unsampled_states_to_zero=False, psi_fn=psi_fn, max_table=M + room)
    finally:
        del ham.local_energy
    assert len(blocks) >= 3 and blocks[0][0] == 0 and sum(n for _, n in blocks) == M, blocks
    assert all(b0 + n0 == b1 for (b0, n0), (b1, _) in zip(blocks, blocks[1:])), blocks
    assert torch.equal(split, whole)
    # a single row that does not fit is an error that names the row
    with pytest.raises(NaqsError, match=r"row \d+: more than 0 connected states outside the table of %d \(at least [1-9]" % M):
        opt.calculate_local_energy(keys, set_unsampled_states_to_zero=False, psi_fn=psi_fn, max_table=M)


# ------------------------------------------------------------------------------------------------------ eigenstate
@pytest.mark.parametrize("mol", ["LiH", "H2O"])
def test_exact_local_energy_is_constant_at_an_eigenstate(env, mol):
    """test_exact_eigenvector_gives_constant_local_energy on every other state of the space: with psi evaluated on the
    connected states outside the table every row gives E0; the truncated mode on the same table does not."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    h = golden(f"ham_{mol}.npz")
    kat = json.load(open(os.path.join(GOLDEN, "kat.json")))
    ham = dev_ham(env, mol)
    space = all_keys(int(h["n_qubits"]), int(h["n_alpha"]), int(h["n_beta"]))
    k = env["H"].keys_to_device(space, ham.device)
    hij = ham.dense_hij(k).cpu().numpy()
    uxy = np.unique(h["xy"])
    j = space[:, None] ^ uxy[None, :]
    pos = np.searchsorted(space, j)
    pos[pos == len(space)] = 0
    hit = space[pos] == j
    rows = np.broadcast_to(np.arange(len(space))[:, None], j.shape)[hit]
    Hm = sp.csr_matrix((hij[hit], (rows, pos[hit])), shape=(len(space),) * 2)
    w, v = spla.eigsh(Hm, k=1, which="SA")
    assert abs(w[0] - kat["fci"][mol]) < 1e-8
    psi = v[:, 0] * np.exp(0.7j)
    tab = np.arange(0, len(space), 2)
    big = np.abs(psi[tab]) > 1e-6 * np.abs(psi).max()
    with np.errstate(divide="ignore"):
        table = np.stack([np.log(np.abs(psi)), np.angle(psi)], -1)
    opt = _bare_optimizer(ham)
    keys = torch.as_tensor(space[tab].astype(np.int64), device=ham.device)
    psi_s = torch.as_tensor(np.stack([psi[tab].real, psi[tab].imag], -1), device=ham.device)
    e = _complex(opt.calculate_local_energy(keys, psi=psi_s, set_unsampled_states_to_zero=False, psi_fn=_lookup(space, table, ham.device)))
    t = _complex(opt.calculate_local_energy(keys, psi=psi_s))
    bound = 1e-6 * max(1.0, abs(w[0]))
    worst, worst_t = np.max(np.abs(e[big] - w[0])), np.max(np.abs(t[big] - w[0]))
    print(f"[exact_eloc] {mol} eigenstate, every other state: exact mode off E0 by {worst:.2e} Ha, truncated by {worst_t:.2e} Ha")
    assert worst < bound
    assert worst_t > bound                                      # the power of the check: the old mode cannot pass it


# ------------------------------------------------------------------------------------------------- psi from the network
def _net(mol, fallback, seed=2):
    """Random-parameter networks on LiH (12 qubits, grad_reference.SECTORS) and H2O STO-3G (14 qubits, (5, 5): SECTORS has
    no entry of that size, the network is built by sector_net's recipe): the published single-phase shape (HIP kernels), or
    -comb_amp_phase with the aggregate phase (LiH_combampphase's shape: PyTorch modules, the announced fallback)."""
    from naqs_amd.hilbert import Encoding, Hilbert
    from naqs_amd.wavefunction import NAQSComplex_NADE_orbitals
    from test_nade import ELECTRONS
    N, na, nb = ELECTRONS[mol]
    hil = Hilbert.get(N, na, nb, encoding=Encoding.SIGNED, make_basis=True)
    torch.manual_seed(seed)
    if fallback:
        wf = NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, amp_hidden_size=[32], phase_hidden_size=[32],
                                       aggregate_phase=True, combined_amp_phase_blocks=True, n_alpha_electrons=na, n_beta_electrons=nb)
    else:
        wf = NAQSComplex_NADE_orbitals(hil, device="cuda", qubit_ordering=-1, amp_hidden_size=[64], phase_hidden_size=[512, 512],
                                       use_amp_spin_sym=True, use_phase_spin_sym=False, aggregate_phase=False,
                                       n_alpha_electrons=na, n_beta_electrons=nb)
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


@pytest.mark.parametrize("mol", ["LiH", "H2O"])
@pytest.mark.parametrize("fallback", [False, True])
def test_exact_mode_with_psi_from_the_network(env, mol, fallback, tmp_path, capsys):
    """Half the space sampled; the rows of the whole-space evaluation (log psi of all states from ONE call) are the
    reference.  Two independent float32 evaluations of log psi_k differ from float64 by at most eps each, eps the bound
    tests/test_forward_f64_gpu.py holds the forward to (P LOG_PAIR + LOG_REL |log|psi|| for the modulus, PHASE_REL
    max(PHASE_FLOOR, max |phase|) for the phase), so term j of row i moves by at most 2 eps |H_ij psi_j / psi_i|:
        |dE_i| <= 2 eps sum_j |H_ij psi_j / psi_i|,
    everything on the right evaluated in float64 from the float64 view of the whole-space log psi.
    Measured on an MI355X, worst |dE_i| / bound: 0 in all four cases (the forward is row-independent and deterministic: the
    same key gives the same bits in both calls)."""
    from test_forward_f64_gpu import LOG_PAIR, LOG_REL, PHASE_FLOOR, PHASE_REL
    hil, wf = _net(mol, fallback)
    opt = _opt(mol, wf, tmp_path)
    assert (wf.fused() is None) == fallback
    ham = opt.pauli_hamiltonian
    h = golden(f"ham_{mol}.npz")
    space = all_keys(hil.N, hil.N_alpha, hil.N_beta)
    kd = env["H"].keys_to_device(space, ham.device)
    with torch.no_grad():
        lp_full = (wf.log_psi(hil.idx2state(kd)) if fallback else wf.fused(need_phase=True).log_psi(kd)).reshape(-1, 2).double()
    e_full = _complex(ham.local_energy(kd, lp_full, kind="log_psi"))
    pos = np.random.RandomState(13).permutation(len(space))[:len(space) // 2]
    e = opt.calculate_local_energy(kd[torch.as_tensor(pos, device=ham.device)], set_unsampled_states_to_zero=False, ret_complex=True)
    # the bound, in float64
    lp = lp_full.cpu().numpy()
    P = hil.N // 2
    eps = float(np.max(P * LOG_PAIR + LOG_REL * np.abs(lp[:, 0])) + PHASE_REL * max(PHASE_FLOOR, np.abs(lp[:, 1]).max()))
    hij = np.abs(ham.dense_hij(kd).cpu().numpy())
    uxy = np.unique(h["xy"])
    j = space[:, None] ^ uxy[None, :]
    at = np.searchsorted(space, j)
    at[at == len(space)] = 0
    hit = space[at] == j
    ratio = np.exp(lp[at, 0] - lp[:, None, 0])                  # |psi_j / psi_i|
    s = np.where(hit, hij * ratio, 0.0).sum(1)
    bound = 2.0 * eps * s[pos]
    d = np.abs(e - e_full[pos])
    frac = float(np.max(d / np.maximum(bound, 1e-300)))
    with capsys.disabled():
        print(f"\n[exact_eloc] {mol} {'fallback' if fallback else 'fused'} net: worst |dE| {d.max():.2e} Ha = {frac:.3f} x bound "
              f"(eps {eps:.2e}, bound <= {bound.max():.2e})")
    assert np.all(np.isfinite(e)) and np.all(d <= bound), frac
    # and the truncated mode is a different quantity on this table
    t = opt.calculate_local_energy(kd[torch.as_tensor(pos, device=ham.device)], ret_complex=True)
    assert np.max(np.abs(t - e_full[pos])) > bound.max()


# ---------------------------------------------------------------------------------------------------- evaluate_energy
def test_evaluate_energy_on_the_whole_space_and_on_half(env, tmp_path):
    hil, wf = _net("H2O", fallback=False)
    opt = _opt("H2O", wf, tmp_path)
    space = all_keys(14, 5, 5)
    kd = env["H"].keys_to_device(space, opt.device)
    lp = wf.fused(need_phase=True).log_psi(kd).double()
    w = (2.0 * lp[:, 0]).exp()
    w = w / w.sum()
    want = opt.calculate_energy(normalise_psi=True)
    res = opt.evaluate_energy(keys=kd, weights=w)
    assert set(res) == {"E", "Var", "stderr", "n_unq", "n_connected"}
    assert abs(res["E"] - want) <= 1e-9, (res["E"], want)
    assert res["n_connected"] == 0 and res["n_unq"] == 441 and res["stderr"] is None and res["Var"] >= 0
    # half the table: psi is evaluated outside it; nothing about the run changes
    params = wf.flatten_parameters().clone()
    t_before, steps = opt.optimizer._t, opt.n_steps
    pos = torch.as_tensor(np.random.RandomState(2).permutation(441)[:220], device=opt.device)
    wh = w[pos] / w[pos].sum()
    half = opt.evaluate_energy(keys=kd[pos], weights=wh)
    assert np.isfinite([half["E"], half["Var"]]).all() and half["n_connected"] > 0 and half["n_unq"] == 220
    trunc = opt.evaluate_energy(keys=kd[pos], weights=wh, exact=False)
    assert trunc["n_connected"] == 0 and abs(trunc["E"] - half["E"]) > 1e-6
    # exact rows of the half table are the whole-space rows: the estimate is the same weighted mean
    e_full = opt.pauli_hamiltonian.local_energy(kd, lp, kind="log_psi")
    assert abs(half["E"] - float((wh * e_full[pos, 0]).sum())) <= 1e-9
    # a drawn table carries an error bar
    drawn = opt.evaluate_energy(n_samps=10 ** 5)
    assert drawn["stderr"] is not None and abs(drawn["stderr"] - np.sqrt(drawn["Var"] / 1e5)) < 1e-12 and drawn["n_unq"] > 10
    assert abs(drawn["E"] - want) < 6 * drawn["stderr"] + 1e-9
    assert torch.equal(params, wf.flatten_parameters()) and opt.optimizer._t == t_before and opt.n_steps == steps


def test_exact_eloc_switch_of_the_command_line(tmp_path, capsys):
    sys.path.insert(0, PKG)
    from experiments import _base
    common = ["-m", os.path.join(GOLDEN, "ham_LiH.npz"), "-single_phase", "-n_hid", "16", "-n_hid_phase", "32", "-n_layer_phase", "2",
              "-n_samps", "100000", "-n_unq_samps_min", "10", "-n_unq_samps_max", "100000", "-n_train", "6", "-output_freq", "2",
              "-lr", "0.001", "-s", "7"]
    res = _base.run(n_hid=128, argv=common + ["-o", str(tmp_path / "on"), "-exact_eloc"])
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("VMC energy with exact local energies: ")]
    assert len(line) == 1 and " Ha (" in line[0] and "sampled + " in line[0] and line[0].endswith("connected states)"), out[-2000:]
    summary = open(tmp_path / "on" / "summary.txt").read().splitlines()
    assert summary[-1] == line[0]
    r = res[0]
    assert np.isfinite(r["e_exact"]) and r["e_exact_stderr"] >= 0 and r["e_exact"] > r["fci"] - 6 * r["e_exact_stderr"] - 1e-9
    assert "\texact_eloc : True" in out
    res = _base.run(n_hid=128, argv=common + ["-o", str(tmp_path / "off")])
    out = capsys.readouterr().out
    assert "exact local energies" not in out and "exact_eloc :" not in out
    assert "exact local energies" not in open(tmp_path / "off" / "summary.txt").read()
    assert "e_exact" not in res[0] and "e_exact_stderr" not in res[0]
