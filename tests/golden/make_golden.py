"""Generate the golden vectors in ``tests/golden/*.npz`` from the REFERENCE itself.

TEST INFRASTRUCTURE — runs only in the build container (needs ``/root/reference``);
``python tests/golden/make_golden.py`` regenerates every fixture.  The reference is
imported through ``ref_harness`` (scratch copy + shims); only
arrays (inputs and the reference's outputs) are written — no reference source.

Fixtures
  ham_<mol>.npz    packed Pauli terms exactly as hamiltonian.py:373-430 / :248-252 produce them
  eloc_<mol>.npz   fixed sample sets + psi -> calculate_local_energy (energy.py:219-263), the
                   complex128 result *before* the float32 cast and the float32 tensor returned,
                   plus the inner-ring intermediates (popcount_parity, get_Hij_cy, H_sub CSR,
                   sparse_dense_mv) on a small subset
  nade_<mol>.npz   NADE state_dict, states -> log_psi (wavefunction.py:167-183), one sampler draw
                   (statistical use only) and the scalars / gradients of one _SGD_step
                   (energy.py:273-377)
  kat.json         physics known answers (FCI energies through the reference path) + timings
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

OUT = os.environ.get("NAQS_GOLDEN_OUT", HERE)      # (a scratch directory when re-deriving fixtures to compare)

rh.setup()

import torch  # noqa: E402
from torch import nn  # noqa: E402
import scipy.sparse.linalg as spla  # noqa: E402

import src.utils.complex as cplx  # noqa: E402
from src.naqs.network.activations import SoftmaxLogProbAmps  # noqa: E402
from src.naqs.network.base import InputEncoding, NadeMasking  # noqa: E402
from src.naqs.wavefunction import NAQSComplex_NADE_orbitals  # noqa: E402
from src.optimizer.energy import PartialSamplingOptimizer  # noqa: E402
from src.optimizer.hamiltonian import PauliHamiltonian, _PauliHamiltonianDynamic  # noqa: E402
from src.utils.hamiltonian_math import get_Hij_cy, popcount_parity  # noqa: E402
from src.utils.hilbert import Encoding, Hilbert  # noqa: E402
from src.utils.sparse_math import sparse_dense_mv  # noqa: E402
from src.utils.system import set_global_seed  # noqa: E402

N2_SWEEP = ["N2_0.75", "N2_0.9", "N2_1.05", "N2_1.2", "N2_1.35", "N2_1.5", "N2_1.65", "N2_1.8",
            "N2_1.95", "N2_2.1", "N2_2.25"]


def electrons(mol):
    key = "N2" if mol.startswith("N2") else mol
    if key in rh.ELECTRONS:
        return rh.ELECTRONS[key]
    v = molecule_scalars(mol)                       # (n_alpha, n_beta) with m_s = S, as experiments/_base.py:101-123 restricts
    n, mult = int(v["n_electrons"]), int(v["multiplicity"])
    return (n + mult - 1) // 2, (n - mult + 1) // 2


def make_hilbert(mol, qh):
    N = rh.n_qubits_of(qh)
    na, nb = electrons(mol)
    return Hilbert.get(N, na, nb, encoding=Encoding.SIGNED, make_basis=True)


class _StubHilbert:
    """Just enough of _HilbertRestricted for __calc_coupling_info (Li2O: the real one needs >25 GB)."""

    def __init__(self, N):
        self.N, self.N_occ, self.encoding = N, 0, Encoding.SIGNED
        self._idx_np_dtype = np.int16 if N < 16 else (np.int32 if N < 30 else np.int64)
        self._idx_torch_dtype = {np.int16: torch.int16, np.int32: torch.int32,
                                 np.int64: torch.int64}[self._idx_np_dtype]
        self._idx_basis_vec = torch.tensor([2 ** n for n in range(N)], dtype=self._idx_torch_dtype)
        self.size = 1

    def to_idx_array(self, idx):
        if torch.is_tensor(idx):
            idx = idx.numpy()
        return np.asarray(idx).astype(self._idx_np_dtype)

    def get_idx_dtype(self, kind="torch"):
        return self._idx_np_dtype if kind in ("np", "numpy") else self._idx_torch_dtype

    def full2restricted_idx(self, idx):
        return idx


def molecule_scalars(mol):
    """n_electrons / multiplicity / reference energies from the molecule's HDF5 file (read with this repo's
    own minimal reader — h5py is not installed)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "naqs-for-quantum-chemistry_amd"))
    from naqs_amd.hdf5_lite import read_hdf5
    v = read_hdf5(os.path.join(rh.REFERENCE, "molecules", mol, f"{mol}.hdf5"),
                  keys=["n_electrons", "multiplicity", "hf_energy", "ccsd_energy", "fci_energy"])
    return {k: np.float64(v[k]) if isinstance(v[k], float) else np.int64(v[k]) for k in v}


def pack_hamiltonian(mol, ph, hilbert_N, out):
    na, nb = electrons(mol)
    np.savez_compressed(
        out, **molecule_scalars(mol),
        n_qubits=np.int64(hilbert_N), n_alpha=np.int64(na), n_beta=np.int64(nb),
        xy=ph.XY_sites_idx.astype(np.uint64), yz=ph.YZ_sites_idx.astype(np.uint64),
        coeff=ph.couplings.squeeze().astype(np.float64),
        unique_xy=ph._unique_XY_sites_idx.astype(np.uint64),
        unique2all_xy=ph._unique2all_XY_sites_idx.astype(np.int64),
        unique_yz=ph._unique_YZ_sites_idx.astype(np.uint64),
        unique2all_yz=ph._unique2all_YZ_sites_idx.astype(np.int64))


def gen_ham_only(mol):
    """Term packing through the reference's own pre-processing, with a stub Hilbert space."""
    qh = rh.load_qubit_hamiltonian(mol)
    N = rh.n_qubits_of(qh)
    ph = object.__new__(_PauliHamiltonianDynamic)
    ph.hilbert, ph.qubit_hamiltonian = _StubHilbert(N), qh
    ph.n_excitations_max, ph.dtype, ph.verbose = None, np.float64, False
    ph.XY_sites_idx, ph.YZ_sites_idx, ph.couplings = ph._PauliHamiltonianDynamic__calc_coupling_info()
    ph._unique_XY_sites_idx, ph._unique2all_XY_sites_idx = np.unique(ph.XY_sites_idx, return_inverse=True)
    ph._unique_YZ_sites_idx, ph._unique2all_YZ_sites_idx = np.unique(ph.YZ_sites_idx, return_inverse=True)
    pack_hamiltonian(mol, ph, N, os.path.join(OUT, f"ham_{mol}.npz"))
    print(f"[ham] {mol}: N={N} K={len(ph.couplings)} Kxy={len(ph._unique_XY_sites_idx)} "
          f"Kyz={len(ph._unique_YZ_sites_idx)}")


def reference_packing(mol):
    qh = rh.load_qubit_hamiltonian(mol)
    N = rh.n_qubits_of(qh)
    ph = object.__new__(_PauliHamiltonianDynamic)
    ph.hilbert, ph.qubit_hamiltonian = _StubHilbert(N), qh
    ph.n_excitations_max, ph.dtype, ph.verbose = None, np.float64, False
    xy, yz, c = ph._PauliHamiltonianDynamic__calc_coupling_info()
    return N, np.asarray(xy).astype(np.uint64), np.asarray(yz).astype(np.uint64), np.asarray(c).squeeze().astype(np.float64)


def gen_packing_hashes():
    """SHA-256 of the reference's own term packing (hamiltonian.py:373-430: xy | yz | coeff, little-endian uint64 / uint64 /
    float64, reference term order) for EVERY molecule folder it ships with a qubit-Hamiltonian pickle ->
    packing_sha256.json; tests/test_packing.py holds naqs_amd.packing to them (build container: needs the folders)."""
    import hashlib
    out = {}
    root = os.path.join(rh.REFERENCE, "molecules")
    for mol in sorted(os.listdir(root)):
        if not os.path.exists(os.path.join(root, mol, f"{mol}_qubit_hamiltonian.pkl")):
            continue
        N, xy, yz, c = reference_packing(mol)
        h = hashlib.sha256(xy.tobytes() + yz.tobytes() + c.tobytes()).hexdigest()
        out[mol] = {"n_qubits": int(N), "K": int(len(c)), "Kxy": int(len(np.unique(xy))), "Kyz": int(len(np.unique(yz))),
                    "sha256": h}
        print(f"[packing] {mol}: N={N} K={len(c)} {h[:16]}")
    with open(os.path.join(OUT, "packing_sha256.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    gen_packing_terms(sorted(out))


def gen_packing_terms(mols):
    """The Pauli terms of the same qubit-Hamiltonian pickles as arrays -> packing_terms.npz, so that tests/test_packing.py
    can pack every molecule without the folders: per molecule `<mol>:ops` (uint8 [K, n_qubits], 0/1/2/3 = I/X/Y/Z, one row
    per term in the pickle's term order), `<mol>:coeff` (complex128 [K]) and `<mol>:electrons` ([n_electrons, multiplicity]
    from the HDF5 file).  Each molecule's terms are rebuilt from the arrays and checked against the pickle, order included."""
    arrays = {}
    for mol in mols:
        qh = rh.load_qubit_hamiltonian(mol)
        N = rh.n_qubits_of(qh)
        ops = np.zeros((len(qh.terms), N), np.uint8)
        for i, term in enumerate(qh.terms):
            for q, op in term:
                ops[i, q] = "IXYZ".index(op)
        coeff = np.array([complex(c) for c in qh.terms.values()], np.complex128)
        rebuilt = [(tuple((q, "IXYZ"[o]) for q, o in enumerate(row) if o), c) for row, c in zip(ops.tolist(), coeff)]
        assert rebuilt == [(tuple(k), complex(c)) for k, c in qh.terms.items()], mol
        v = molecule_scalars(mol)
        arrays[f"{mol}:ops"], arrays[f"{mol}:coeff"] = ops, coeff
        arrays[f"{mol}:electrons"] = np.array([v["n_electrons"], v["multiplicity"]], np.int64)
    np.savez_compressed(os.path.join(OUT, "packing_terms.npz"), **arrays)


def gen_li2o_subset():
    """Li2O (30 qubits, int64 idx dtype): the reference's Hilbert/update_H cannot be instantiated here
    (2^30-entry look-up tables), but its Cython kernels can be driven directly — the pipeline of
    update_H (hamiltonian.py:301-337) on a clustered sample set with the reference's own
    popcount_parity / get_Hij_cy / sparse_dense_mv, the particle-number test standing in for the 2^N table."""
    from scipy.sparse import csr_matrix
    mol = "Li2O"
    qh = rh.load_qubit_hamiltonian(mol)
    N = rh.n_qubits_of(qh)
    ph = object.__new__(_PauliHamiltonianDynamic)
    ph.hilbert, ph.qubit_hamiltonian = _StubHilbert(N), qh
    ph.n_excitations_max, ph.dtype, ph.verbose = None, np.float64, False
    XY, YZ, cpl = ph._PauliHamiltonianDynamic__calc_coupling_info()
    uXY, u2aXY = np.unique(XY, return_inverse=True)
    uYZ, u2aYZ = np.unique(YZ, return_inverse=True)
    # clustered samples: a random walk over connected physical states from one determinant
    rs = np.random.RandomState(2024)
    amask, bmask = sum(1 << q for q in range(0, N, 2)), sum(1 << q for q in range(1, N, 2))
    base = sum(1 << q for q in range(14))
    keys, frontier = {base}, [base]
    while len(keys) < 1500:
        k = frontier[rs.randint(len(frontier))]
        j = k ^ int(uXY[rs.randint(len(uXY))])
        if bin(j & amask).count("1") == 7 and bin(j & bmask).count("1") == 7 and j not in keys:
            keys.add(j)
            frontier.append(j)
    keys = np.sort(np.array(list(keys), np.int64))
    M, Kxy = len(keys), len(uXY)
    P = popcount_parity(np.bitwise_and(keys[:, None], uYZ[None, :]))
    Hij = get_Hij_cy(keys, uXY, u2aXY, P, u2aYZ, cpl.squeeze())
    j_full = np.bitwise_xor(keys[:, None], uXY[None, :]).ravel()
    pos = np.searchsorted(keys, j_full)
    pos[pos == M] = 0
    hit = keys[pos] == j_full                      # sampled (hence physical) connected states only
    rows = np.repeat(np.arange(M), Kxy)[hit]
    H = csr_matrix((Hij[hit], (rows, pos[hit])), shape=(M, M))
    log_psi, psi = synthetic_psi(M, 1.5, seed=99)
    v = cplx.torch_to_numpy(psi)
    e = (sparse_dense_mv(H, v) / v).conj()
    np.savez_compressed(os.path.join(OUT, "eloc_Li2O_subset.npz"), keys=keys.astype(np.uint64),
                        psi_f32=psi.numpy(), log_psi_f32=log_psi.numpy(), eloc_c128=e, nnz=np.int64(H.nnz))
    print(f"[eloc] Li2O subset: M={M} nnz={H.nnz} <E_loc>={e.real.mean():.6f}")


def wavefunction_args(na, nb, n_hid, n_hid_phase, n_layer_phase, masking=NadeMasking.PARTIAL, **overrides):
    # experiments/_base.py:150-187 with the published flags (batch_train.sh:14)
    return dict(_wavefunction_args(na, nb, n_hid, n_hid_phase, n_layer_phase, masking), **overrides)


def _wavefunction_args(na, nb, n_hid, n_hid_phase, n_layer_phase, masking):
    return dict(qubit_ordering=-1, masking=masking, num_lut=0, input_encoding=InputEncoding.BINARY,
                amp_hidden_size=[n_hid], amp_hidden_activation=nn.ReLU, amp_bias=True,
                phase_hidden_size=[n_hid_phase] * n_layer_phase, phase_hidden_activation=nn.ReLU,
                phase_bias=True, combined_amp_phase_blocks=False, use_amp_spin_sym=True,
                use_phase_spin_sym=False, aggregate_phase=False, amp_batch_norm=False,
                phase_batch_norm=False, batch_norm_momentum=1, amp_activation=SoftmaxLogProbAmps,
                phase_activation=None, n_alpha_electrons=na, n_beta_electrons=nb)


def make_optimizer(wf, qh, na, nb, n_samples, grad_clip_factor=None):
    # experiments/_base.py:209-246
    return PartialSamplingOptimizer(
        n_samples=n_samples, n_samples_max=1e12, n_unq_samples_min=10, n_unq_samples_max=1e5,
        log_exact_energy=False, wavefunction=wf, qubit_hamiltonian=qh, pre_compute_H=False,
        n_electrons=na + nb, n_alpha_electrons=na, n_beta_electrons=nb, n_fixed_electrons=None,
        n_excitations_max=None, reweight_samples_by_psi=False, normalise_psi=True,
        normalize_grads=False, grad_clip_factor=grad_clip_factor, grad_clip_memory_length=50,
        optimizer=torch.optim.Adam,
        optimizer_args=[{'lr': 1e-3, 'betas': (0.9, 0.99), 'weight_decay': 0, 'eps': 1e-15,
                         'amsgrad': False}, {'lr': 1e-2}],
        save_loc="/tmp/golden_out", pauli_hamiltonian_fname=None, overwrite_pauli_hamiltonian=True,
        pauli_hamiltonian_dtype=np.float64, verbose=False)


def synthetic_psi(M, sigma, seed=4321):
    """SURVEY 8d recipe: log|psi| ~ N(-ln(M)/2, sigma), phase ~ U[0, 2pi); float32 like the reference."""
    rs = np.random.RandomState(seed)
    la = rs.normal(-0.5 * np.log(M), sigma, size=M)
    ph = rs.uniform(0, 2 * np.pi, size=M)
    log_psi = torch.tensor(np.stack([la, ph], -1), dtype=torch.float32)
    return log_psi, cplx.exp(log_psi)            # psi exactly as _SGD_step builds it (energy.py:310)


def fresh_pauli(opt):
    """A cold _PauliHamiltonianDynamic, built the way OptimizerBase.__init__ does (energy.py:115-125)."""
    restricted = opt.hilbert.get_subspace(ret_states=False, ret_idxs=True, **opt.subspace_args)
    return PauliHamiltonian.get(opt.hilbert, opt.qubit_hamiltonian, hamiltonian_fname=None,
                                restricted_idxs=restricted, verbose=False, n_excitations_max=None,
                                dtype=np.float64)


def nade_vectors(wf, opt, hil, all_keys, n_draw=None):
    """state_dict, teacher-forced log psi / conditionals on a fixed state set, one sampler draw (statistical use
    only) and the scalars / gradients / parameters of the reference's own _SGD_step on that draw."""
    nd = {}
    for k, v_ in wf.model.state_dict().items():
        nd["sd:" + k] = v_.detach().numpy().copy()
    B = min(512, len(all_keys))
    sel = np.sort(np.random.RandomState(3).choice(len(all_keys), B, replace=False))
    states_eval = hil.basis_states[sel]
    with torch.no_grad():
        lp_eval = wf.log_psi(states_eval).numpy()
        cond = wf._evaluate_log_psi(states_eval, gather_state=False).numpy()   # [B, N/2, 4, 2]
    nd.update(eval_states=states_eval.numpy(), eval_keys=all_keys[sel].astype(np.uint64),
              eval_log_psi=lp_eval, eval_cond=cond)

    opt.pauli_hamiltonian = fresh_pauli(opt)
    if n_draw is None:
        n_draw = 2000 if len(all_keys) < 1000 else 200000
    states, counts, probs, log_psi = wf.sample(n_draw)
    idx = hil.state2idx(states)
    nd.update(samp_n=n_draw, samp_states=states.numpy(), samp_counts=counts.numpy(),
              samp_probs=probs.detach().numpy(), samp_log_psi=log_psi.detach().numpy(),
              samp_keys=idx.squeeze().numpy().astype(np.uint64))
    weights = counts.float() / counts.sum().float()
    e_loc = opt.calculate_local_energy(idx.squeeze(), psi=cplx.exp(log_psi.detach()))
    e128 = opt.calculate_local_energy(idx.squeeze(), psi=cplx.exp(log_psi.detach()), ret_complex=True)
    w2 = weights.unsqueeze(-1)
    e_corr = e_loc - (w2 * e_loc).sum(axis=0)
    loss = 2 * cplx.real(w2 * cplx.scalar_mult(log_psi, e_corr)).sum(axis=0)
    grads = {}
    real_step = opt.optimizer.step

    def capture_step(*a, **k):
        for name, p in wf.model.named_parameters():
            grads[name] = p.grad.detach().numpy().copy()
        return real_step(*a, **k)

    opt.optimizer.step = capture_step
    E, Var = opt._SGD_step(states, idx, log_psi, sample_weights=weights.clone())
    opt.optimizer.step = real_step
    nd.update(sgd_eloc_f32=e_loc.numpy(), sgd_eloc_c128=e128, sgd_loss=np.float32(loss.item()),
              sgd_E=np.float64(E), sgd_Var=np.float64(Var))
    for k, g in grads.items():
        nd["grad:" + k] = g
    for k, v_ in wf.model.state_dict().items():
        nd["sd_after:" + k] = v_.detach().numpy().copy()
    return nd


def gen_molecule(mol, M_sets, nade_cfg, seed=111, kat=None, time_it=False):
    set_global_seed(seed)
    qh = rh.load_qubit_hamiltonian(mol)
    na, nb = electrons(mol)
    hil = make_hilbert(mol, qh)
    N = hil.N
    wf = NAQSComplex_NADE_orbitals(hil, **wavefunction_args(na, nb, *nade_cfg))
    opt = make_optimizer(wf, qh, na, nb, n_samples=1000)
    ph = opt.pauli_hamiltonian
    pack_hamiltonian(mol, ph, N, os.path.join(OUT, f"ham_{mol}.npz"))
    all_keys = hil.restricted2full_basis_idxs.numpy().astype(np.int64)

    # ---------------- E_loc goldens on fixed synthetic sample sets ----------------
    out = {}
    for tag, (M, sigma) in M_sets.items():
        keys = np.sort(np.random.RandomState(1234).choice(all_keys, M, replace=False))
        log_psi, psi = synthetic_psi(M, sigma)
        opt.pauli_hamiltonian = fresh_pauli(opt)
        idx = hil.to_idx_tensor(keys)
        e128 = opt.calculate_local_energy(idx, psi=psi, ret_complex=True)
        e32 = opt.calculate_local_energy(idx, psi=psi, ret_complex=False).numpy()
        out.update({f"{tag}_keys": keys.astype(np.uint64), f"{tag}_log_psi_f32": log_psi.numpy(),
                    f"{tag}_psi_f32": psi.numpy(), f"{tag}_eloc_c128": e128, f"{tag}_eloc_f32": e32})
        print(f"[eloc] {mol}/{tag}: M={M} <E_loc>={e128.real.mean():.6f}")

    # ---------------- inner ring on a small subset ----------------
    Ms = min(48, len(all_keys) // 2)
    keys_s = np.sort(np.random.RandomState(99).choice(all_keys, Ms, replace=False))
    idx_s = hil.to_idx_array(keys_s)
    P_bits = np.bitwise_and(idx_s[:, None], ph._unique_YZ_sites_idx[None, :])
    P = popcount_parity(P_bits)
    Hij = get_Hij_cy(idx_s, ph._unique_XY_sites_idx, ph._unique2all_XY_sites_idx, P,
                     ph._unique2all_YZ_sites_idx, ph.couplings.squeeze())
    opt.pauli_hamiltonian = fresh_pauli(opt)
    opt.pauli_hamiltonian.update_H(hil.to_idx_tensor(keys_s), check_unseen=True, assume_unique=True)
    Hs = opt.pauli_hamiltonian.get_H(hil.to_idx_tensor(keys_s)).tocsr()
    Hs.sort_indices()
    _, psi_s = synthetic_psi(Ms, 1.0, seed=7)
    v = cplx.torch_to_numpy(psi_s)
    mv = sparse_dense_mv(Hs, v)
    out.update(dict(ring_keys=keys_s.astype(np.uint64), ring_P=np.asarray(P), ring_Hij=np.asarray(Hij),
                    ring_csr_data=Hs.data, ring_csr_indices=Hs.indices.astype(np.int32),
                    ring_csr_indptr=Hs.indptr.astype(np.int32), ring_v=v, ring_mv=mv))
    # popcount_parity dtype coverage (hamiltonian_math.pyx:455-484)
    rs = np.random.RandomState(5)
    for dt in (np.int16, np.int32, np.int64):
        arr = rs.randint(0, np.iinfo(dt).max, size=(7, 33), dtype=np.int64).astype(dt)
        out[f"pp_in_{np.dtype(dt).name}"] = arr
        out[f"pp_out_{np.dtype(dt).name}"] = np.asarray(popcount_parity(arr))
    np.savez_compressed(os.path.join(OUT, f"eloc_{mol}.npz"), **out)

    # ---------------- NADE: log_psi, sampler draw, one SGD step ----------------
    nd = {"cfg_n_hid": nade_cfg[0], "cfg_n_hid_phase": nade_cfg[1], "cfg_n_layer_phase": nade_cfg[2],
          "seed": seed}
    nd.update(nade_vectors(wf, opt, hil, all_keys))
    np.savez_compressed(os.path.join(OUT, f"nade_{mol}.npz"), **nd)
    print(f"[nade] {mol}: n_unq={len(nd['samp_keys'])} E={nd['sgd_E']:.6f} Var={nd['sgd_Var']:.6f} "
          f"loss={nd['sgd_loss']:.6e}")

    # ---------------- physics known answer: FCI through the reference path ----------------
    if kat is not None:
        opt.pauli_hamiltonian = fresh_pauli(opt)
        H = opt.pauli_hamiltonian.update_H(hil.to_idx_tensor(all_keys), check_unseen=False,
                                           assume_unique=True)
        w = spla.eigsh(H.astype(np.float64), k=1, which="SA", return_eigenvectors=False)
        kat.setdefault("fci", {})[mol] = float(w[0])
        kat.setdefault("nnz", {})[mol] = int(H.nnz)
        print(f"[kat] {mol}: E_FCI={w[0]:.12f} nnz={H.nnz}")

    if time_it:
        tag = list(M_sets)[-1]
        keys = out[f"{tag}_keys"].astype(np.int64)
        psi = torch.tensor(out[f"{tag}_psi_f32"])
        idx = hil.to_idx_tensor(keys)
        cold = []
        for _ in range(7):
            opt.pauli_hamiltonian = fresh_pauli(opt)
            t = time.perf_counter()
            opt.calculate_local_energy(idx, psi=psi)
            cold.append(time.perf_counter() - t)
        warm = []
        for _ in range(10):
            t = time.perf_counter()
            opt.calculate_local_energy(idx, psi=psi)
            warm.append(time.perf_counter() - t)
        kat.setdefault("timing", {})[mol] = {
            "M": int(len(keys)), "threads": int(os.environ.get("OMP_NUM_THREADS", os.cpu_count())),
            "cold_s_median": float(np.median(cold[2:])), "warm_s_median": float(np.median(warm)),
            "where": "build container, reference calculate_local_energy via ref_harness"}
        print("[time]", kat["timing"][mol])


# ------------------------------------------------------------------------------------------------------------
# round 2: the ansatz variants the reference's scripts run, the sweep geometries, and the small compat fixtures
# ------------------------------------------------------------------------------------------------------------
VARIANTS = {
    # tag: (wavefunction_args overrides, (n_hid, n_hid_phase, n_layer_phase), masking)
    # experiments/run.py:11-31 defaults: -n_hid 128 -n_layer 1, phase blocks like the amplitude ones, every block
    # contributes a phase (aggregate_phase=True, nade.py:556-569)
    "aggphase": (dict(aggregate_phase=True), (128, 128, 1), NadeMasking.PARTIAL),
    # batch_train_no_amp_sym.sh:14
    "noampsym": (dict(use_amp_spin_sym=False), "small", NadeMasking.PARTIAL),
    # batch_train_no_mask.sh:14 / batch_train_full_mask.sh:14 (the N2 sweep, N2_energy_surface.sh:5-8)
    "nomask": (dict(), "small", NadeMasking.NONE),
    "fullmask": (dict(), None, NadeMasking.FULL),
    "fullmask_noampsym": (dict(use_amp_spin_sym=False), None, NadeMasking.FULL),
    # round 4: the live options no published script uses (experiments/_base.py:533-541): -phase_sym (nade.py:281, 597-610)
    # and -comb_amp_phase (nade.py:257-262, 294-303, 555: one block per pair emits amplitude AND phase outputs; it forces
    # the phase symmetry to follow the amplitude symmetry) on run.py's default aggregate-phase ansatz
    "phasesym": (dict(use_phase_spin_sym=True), None, NadeMasking.PARTIAL),
    "phasesym_agg": (dict(use_phase_spin_sym=True, aggregate_phase=True), (32, 32, 1), NadeMasking.PARTIAL),
    "combampphase": (dict(combined_amp_phase_blocks=True, aggregate_phase=True), (32, 32, 1), NadeMasking.PARTIAL),
    # -qo 1 (experiments/_base.py:35; wavefunction.py:56-83): model pair n is orbital pair n, not the default reversal
    "qo1": (dict(qubit_ordering=1), None, NadeMasking.PARTIAL),
}
PUBLISHED_CFG = {"LiH": (64, 32, 2), "H2O": (64, 32, 2), "CH2": (64, 32, 2)}        # small phase nets for the small fixtures; else 64/512x2
SMALL_CFG = {"N2": (64, 128, 2)}                                 # keeps the fixture small where the 512-wide phase net is not the point


def gen_variant(mol, tag, seed=111, with_eloc=None):
    """nade_<mol>_<tag>.npz (+ eloc_<mol>.npz for molecules that do not have one yet, ``with_eloc`` = {name: (M, sigma)})."""
    over, cfg, masking = VARIANTS[tag]
    if cfg == "small":
        cfg = SMALL_CFG.get(mol)
    if cfg is None:
        cfg = PUBLISHED_CFG.get(mol, (64, 512, 2))
    set_global_seed(seed)
    qh = rh.load_qubit_hamiltonian(mol)
    na, nb = electrons(mol)
    hil = make_hilbert(mol, qh)
    wf = NAQSComplex_NADE_orbitals(hil, **wavefunction_args(na, nb, *cfg, masking=masking, **over))
    opt = make_optimizer(wf, qh, na, nb, n_samples=1000)
    all_keys = hil.restricted2full_basis_idxs.numpy().astype(np.int64)
    if with_eloc:
        out = {}
        for name, (M, sigma) in with_eloc.items():
            keys = np.sort(np.random.RandomState(1234).choice(all_keys, M, replace=False))
            log_psi, psi = synthetic_psi(M, sigma)
            opt.pauli_hamiltonian = fresh_pauli(opt)
            idx = hil.to_idx_tensor(keys)
            e128 = opt.calculate_local_energy(idx, psi=psi, ret_complex=True)
            out.update({f"{name}_keys": keys.astype(np.uint64), f"{name}_log_psi_f32": log_psi.numpy(),
                        f"{name}_psi_f32": psi.numpy(), f"{name}_eloc_c128": e128})
            print(f"[eloc] {mol}/{name}: M={M} <E_loc>={e128.real.mean():.6f}")
        np.savez_compressed(os.path.join(OUT, f"eloc_{mol}.npz"), **out)
    nd = {"cfg_n_hid": cfg[0], "cfg_n_hid_phase": cfg[1], "cfg_n_layer_phase": cfg[2], "seed": seed,
          "cfg_masking": masking.value, "cfg_aggregate_phase": bool(over.get("aggregate_phase", False)),
          "cfg_use_amp_spin_sym": bool(over.get("use_amp_spin_sym", True)),
          "cfg_use_phase_spin_sym": bool(over.get("use_phase_spin_sym", False)),
          "cfg_combined_amp_phase_blocks": bool(over.get("combined_amp_phase_blocks", False)),
          "cfg_qubit_ordering": int(over.get("qubit_ordering", -1))}
    nd.update(nade_vectors(wf, opt, hil, all_keys))
    np.savez_compressed(os.path.join(OUT, f"nade_{mol}_{tag}.npz"), **nd)
    print(f"[nade] {mol}/{tag}: n_unq={len(nd['samp_keys'])} E={nd['sgd_E']:.6f} Var={nd['sgd_Var']:.6f} "
          f"loss={nd['sgd_loss']:.6e}")


def gen_compat_lih(seed=111):
    """compat_LiH.npz + ckpt_LiH/: (a) three _SGD_steps on one fixed sample table with grad_clip_factor = 0.5 (the
    reference constructor default is 3, energy.py:63; 0.5 makes the clip bite from the second step on, :383-395);
    (b) E_loc of the reference when the batch holds all 225 states (the full-sample ordering quirk Q1,
    hamiltonian.py:100-105); (c) a checkpoint written by the reference's own save() (energy.py:409-443,
    wavefunction.py:240-253) after those steps."""
    import shutil
    mol = "LiH"
    set_global_seed(seed)
    qh = rh.load_qubit_hamiltonian(mol)
    na, nb = electrons(mol)
    hil = make_hilbert(mol, qh)
    wf = NAQSComplex_NADE_orbitals(hil, **wavefunction_args(na, nb, 64, 32, 2))
    opt = make_optimizer(wf, qh, na, nb, n_samples=1000, grad_clip_factor=0.5)
    ck_dir = os.path.join(OUT, "ckpt_LiH")
    shutil.rmtree(ck_dir, ignore_errors=True)
    opt.save_loc = ck_dir
    out = {}
    for k, v_ in wf.model.state_dict().items():
        out["sd:" + k] = v_.detach().numpy().copy()
    states, counts, probs, _ = wf.sample(5000)
    idx = hil.state2idx(states)
    out.update(clip_states=states.numpy(), clip_counts=counts.numpy(), clip_factor=np.float64(0.5))
    norms = []
    real_clip = opt._clip_grads

    def spy_clip():
        norms.append(float(torch.norm(torch.stack([p.grad.norm(2) for p in wf.model.parameters()]), 2)))
        return real_clip()

    opt._clip_grads = spy_clip
    for step in range(3):
        log_psi = wf.log_psi(states)
        w = counts.float() / counts.sum().float()
        E, Var = opt._SGD_step(states, idx, log_psi, sample_weights=w.clone())
        out[f"clip_E{step}"] = np.float64(E)
        for k, v_ in wf.model.state_dict().items():
            out[f"clip_sd{step}:" + k] = v_.detach().numpy().copy()
    out["clip_grad_norms"] = np.array(norms)
    opt.n_steps, opt.n_epochs, opt.run_time = 3, 3, 1.25
    from src.optimizer.utils import LogKey
    for step in range(3):
        opt.log[LogKey.E_LOC].append((step + 1, float(out[f"clip_E{step}"])))
    opt.overwrite_pauli_hamiltonian = False                         # (no Hamiltonian cache file to write)
    opt.save(quiet=True)                                            # -> ckpt_LiH/energy_optimizer(.pth, _naqs.pth)

    # Q1: every state of the space in one batch, ascending keys (what the sampler returns with qubit_ordering = -1)
    all_keys = np.sort(hil.restricted2full_basis_idxs.numpy().astype(np.int64))
    log_psi, psi = synthetic_psi(len(all_keys), 1.0, seed=77)
    opt.pauli_hamiltonian = fresh_pauli(opt)
    e_bug = opt.calculate_local_energy(hil.to_idx_tensor(all_keys), psi=psi, ret_complex=True)
    out.update(q1_keys=all_keys.astype(np.uint64), q1_log_psi_f32=log_psi.numpy(), q1_psi_f32=psi.numpy(),
               q1_eloc_c128=e_bug, q1_restricted_order_keys=hil.restricted2full_basis_idxs.numpy().astype(np.uint64))
    np.savez_compressed(os.path.join(OUT, "compat_LiH.npz"), **out)
    print(f"[compat] LiH: clip norms {norms}, E {[float(out[f'clip_E{i}']) for i in range(3)]}, "
          f"Q1 <E_loc>={e_bug.real.mean():.6f}")


def variants():
    for mol in ("LiH", "N2"):
        for tag in ("aggphase", "noampsym"):
            gen_variant(mol, tag)
    gen_variant("N2", "nomask")
    gen_variant("LiH", "fullmask")
    for mol in ("N2_0.75", "N2_2.25"):
        gen_variant(mol, "fullmask", with_eloc={"c2": (10000, 2.0)})
    gen_compat_lih()
    gen_open_shell()


def widen():
    """round 4: -phase_sym / -comb_amp_phase fixtures and the pre-training step (-n_pretrain), LiH"""
    for tag in ("phasesym", "phasesym_agg", "combampphase"):
        gen_variant("LiH", tag)
    gen_pretrain("LiH")


def gen_pretrain(mol, seed=111, n_epochs=3):
    """pretrain_<mol>.npz: `opt.pre_flatten` exactly as experiments/_base.py:284-289 calls it (-n_pretrain n: supervised epochs
    towards the uniform amplitude over the restricted space, energy.py:840-904) — parameters before and after."""
    set_global_seed(seed)
    qh = rh.load_qubit_hamiltonian(mol)
    na, nb = electrons(mol)
    hil = make_hilbert(mol, qh)
    cfg = PUBLISHED_CFG.get(mol, (64, 512, 2))
    wf = NAQSComplex_NADE_orbitals(hil, **wavefunction_args(na, nb, *cfg))
    opt = make_optimizer(wf, qh, na, nb, n_samples=1000)
    nd = {"cfg_n_hid": cfg[0], "cfg_n_hid_phase": cfg[1], "cfg_n_layer_phase": cfg[2], "seed": seed, "n_epochs": n_epochs}
    for k, v_ in wf.model.state_dict().items():
        nd["sd:" + k] = v_.detach().numpy().copy()
    opt.pre_flatten(n_epochs, 1000, optimizer_args={'lr': 1e-3}, output_freq=25, use_sampling=False, max_batch_size=550000,
                    flatten_phase=False)
    for k, v_ in wf.model.state_dict().items():
        nd["sd_after:" + k] = v_.detach().numpy().copy()
    states = hil.basis_states
    with torch.no_grad():
        nd["log_amp_after"] = wf.log_psi(states)[..., 0].numpy()
    nd["target"] = np.float64(np.log(1 / np.sqrt(len(states))))
    np.savez_compressed(os.path.join(OUT, f"pretrain_{mol}.npz"), **nd)
    print(f"[pretrain] {mol}: mean log|psi| after {n_epochs} epochs = {nd['log_amp_after'].mean():.6f} (target {nd['target']:.6f})")


def gen_open_shell():
    """Open-shell molecule restricted to m_s = S (experiments/_base.py:101-123: CH2 is a triplet -> 5 alpha / 3 beta
    electrons, amplitude spin symmetry switched off): network vectors, sampler draw, _SGD_step and E_loc."""
    gen_variant("CH2", "noampsym", with_eloc={"c1": (400, 1.5)})
    gen_variant("CH2", "fullmask_noampsym")


TRAJ_FLAGS = ["-single_phase", "-n1", "-n_layer", "1", "-n_hid", "64", "-n_layer_phase", "2", "-n_hid_phase", "512",
              "-n_train", "10000", "-output_freq", "25", "-save_freq", "-1", "-full_mask_psi"]      # batch_train_full_mask.sh:14


def gen_trajectory(mol, seed=111, threads=4):
    """Whole-run known answer: the reference's own ``experiments/run.py`` entry (``experiments/_base.py:394-659`` ->
    ``PartialSamplingOptimizer.run``, ``energy.py:902-1056``) with the flags of ``batch_train_full_mask.sh`` on one
    geometry of the N2 sweep.  Only the molecule loader (needs openfermion / h5py: replaced by the repository's own
    readers of the same files) and the plotting at the end are stubbed.  Writes ``traj_<mol>_s<seed>.json`` (final
    energies, unique-sample counts along the run, wall time) which ``kat.json`` then indexes."""
    import importlib
    torch.set_num_threads(threads)
    B = importlib.import_module("experiments._base")             # the REFERENCE's (scratch copy first on sys.path) ...
    assert os.path.abspath(B.__file__).startswith(os.path.abspath(rh.SCRATCH)), B.__file__
    sys.path.append(os.path.join(os.path.dirname(os.path.dirname(HERE)), "naqs-for-quantum-chemistry_amd"))
    from naqs_amd import system as repo_system                 # ... the repository's file readers: no openfermion / h5py
    from src.optimizer.utils import LogKey
    made = []

    class Spy(B.PartialSamplingOptimizer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    class _Fig:
        def savefig(self, *a, **k):
            pass

    B.PartialSamplingOptimizer = Spy
    B.load_molecule = lambda fname, hamiltonian_fname=None, verbose=True: repo_system.load_molecule(fname, hamiltonian_fname, verbose)
    B.plot_training = lambda *a, **k: _Fig()
    out = f"/tmp/golden_traj/{mol}_s{seed}"
    argv = ["run", "-o", out, "-m", os.path.join(rh.REFERENCE, "molecules", mol), "-s", str(seed)] + TRAJ_FLAGS
    old_argv, sys.argv = sys.argv, argv
    t0 = time.time()
    try:
        # the keyword defaults of experiments/run.py:3-33, then the command line above on top of them
        B.run(molecule=None, out=None, number=1, lr=-1, n_samps=1e7, n_samps_max=1e12, n_unq_samps_min=1e4, n_unq_samps_max=1e5,
              n_hid=128, n_layer=1, reweight_samples_by_psi=False, n_train=10000, n_pretrain=0, output_freq=25, save_freq=-1,
              load_hamiltonian=False, overwrite_hamiltonian=False, presolve_hamiltonian=False, cont=False, n_excitations_max=-1,
              use_amp_spin_sym=True, use_phase_spin_sym=False, comb_amp_phase=False, aggregate_phase=True, restrict_H=True,
              reset_opt=False)
    finally:
        sys.argv = old_argv
    wall = time.time() - t0
    opt = made[-1]
    e_loc = np.array([e for _, e in opt.log[LogKey.E_LOC]], dtype=np.float64)
    n_unq = np.array([n for _, n in opt.log[LogKey.N_UNIQUE_SAMP]], dtype=np.int64)
    t_run = np.array([t for _, t in opt.log[LogKey.TIME]], dtype=np.float64)
    w = 25
    conv = np.convolve(e_loc, np.ones(w) / w, "valid")
    rec = {"molecule": mol, "seed": seed, "flags": " ".join(TRAJ_FLAGS), "steps": int(len(e_loc)), "threads": threads,
           "wall_s": wall, "train_s": float(t_run[-1]),
           "final_E_loc": float(e_loc[-1]), "mean_last_100": float(e_loc[-100:].mean()), "min_E_loc": float(e_loc.min()),
           "min_sliding_25": float(conv.min()),
           "n_unq_every_500": [int(x) for x in n_unq[::500]], "n_unq_last": int(n_unq[-1]),
           "E_loc_every_500": [float(x) for x in e_loc[::500]],
           "where": "build container, reference experiments/run.py via tests/golden/ref_harness.py"}
    with open(os.path.join(OUT, f"traj_{mol}_s{seed}.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(f"[traj] {mol} seed {seed}: final {rec['final_E_loc']:.8f} mean100 {rec['mean_last_100']:.8f} in {wall:.0f} s")


def main():
    kat = {}
    gen_molecule("LiH", {"c1": (150, 1.0), "half": (100, 2.0)}, (64, 32, 2), kat=kat)
    gen_molecule("H2O", {"c1": (300, 1.0)}, (64, 32, 2), kat=kat)
    gen_molecule("N2", {"small": (2000, 2.0), "c2": (10000, 2.0)}, (64, 512, 2), kat=kat, time_it=True)
    gen_ham_only("Li2O")
    gen_li2o_subset()
    for mol in N2_SWEEP:
        gen_ham_only(mol)
    with open(os.path.join(OUT, "kat.json"), "w") as f:
        json.dump(kat, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("all", "base"):
        main()
    if which in ("all", "variants"):
        variants()
    if which == "widen":
        widen()
    if which == "ordering":             # python make_golden.py ordering   (nade_LiH_qo1.npz)
        gen_variant("LiH", "qo1")
    if which == "compat":
        gen_compat_lih()
    if which == "open-shell":
        gen_open_shell()
    if which == "packing":              # python make_golden.py packing   (every molecule folder; seconds)
        gen_packing_hashes()
    if which == "ham":                  # python make_golden.py ham PH3 H4O2 C2 ...   (packed-term fixtures only)
        for mol in sys.argv[2:]:
            gen_ham_only(mol)
    if which == "trajectory":           # python make_golden.py trajectory N2_2.25 [seed]   (~6 min on 4 threads)
        gen_trajectory(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 111)
    if which == "check-LiH":            # re-derive one base fixture into $NAQS_GOLDEN_OUT (refactoring guard)
        gen_molecule("LiH", {"c1": (150, 1.0), "half": (100, 2.0)}, (64, 32, 2), kat={})
