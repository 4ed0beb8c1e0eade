"""Device-resident Pauli Hamiltonian: the drop-in counterpart of the reference's
``PauliHamiltonian`` (src/optimizer/hamiltonian.py:32-216, :218-370) for the local-energy path.

The reference caches a scipy CSR matrix over the restricted Hilbert space and grows it lazily
(``update_H``); here nothing is cached — ``libnaqs_hip.so`` regenerates matrix elements on the
fly from the packed terms (matrix-free), so ``update_H`` / ``freeze_H`` keep their names and
argument meaning but only validate / record state.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .packing import PackedHamiltonian, pack_qubit_hamiltonian

_KIND = {("psi", torch.float32): _lib.PSI_F32, ("psi", torch.float64): _lib.PSI_F64,
         ("log_psi", torch.float32): _lib.LOGPSI_F32, ("log_psi", torch.float64): _lib.LOGPSI_F64}


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def keys_to_device(keys, device):
    """Any integer array/tensor of bit-string keys -> contiguous device int64 tensor holding the
    uint64 bit pattern (torch has no uint64 arithmetic; only the bits matter)."""
    if isinstance(keys, np.ndarray):
        keys = torch.from_numpy(np.ascontiguousarray(keys).astype(np.uint64).view(np.int64))
    keys = keys.reshape(-1)
    if keys.dtype != torch.int64:
        keys = keys.to(torch.int64)
    return keys.to(device).contiguous()


class DevicePauliHamiltonian:
    """Packed terms on one GPU + the kernels that consume them (handle of ``naqs_ham_create``)."""

    def __init__(self, packed: PackedHamiltonian, device=None):
        self._h = ctypes.c_void_p(None)
        self.last_lanczos_iterations = 0          # products of the most recent lowest_eigenpair call (measurement aid)
        self.last_eig_info = None                 # dict(products, residual, status) of the most recent solver="davidson" call
                                                  # (lowest_eigenpairs: residuals, one per root)
        self._lib = _lib.load_library()           # raises NaqsError when the HIP library is missing
        if not torch.cuda.is_available():
            raise _lib.NaqsError("DevicePauliHamiltonian needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.packed = packed
        xy = np.ascontiguousarray(packed.xy, np.uint64)
        yz = np.ascontiguousarray(packed.yz, np.uint64)
        cf = np.ascontiguousarray(packed.coeff, np.float64)
        st = self._lib.naqs_ham_create(packed.n_qubits, packed.n_alpha, packed.n_beta, packed.K,
                                       xy.ctypes.data, yz.ctypes.data, cf.ctypes.data,
                                       self.device.index, ctypes.byref(self._h))
        _lib.check(st, "naqs_ham_create")
        info = (ctypes.c_int64 * 8)()
        _lib.check(self._lib.naqs_ham_info(self._h, ctypes.byref(info)), "naqs_ham_info")
        self.K, self.Kxy, self.n_qubits = int(info[0]), int(info[1]), int(info[2])
        self.key_bits, self.diag_terms = int(info[5]), int(info[6])

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.naqs_ham_destroy(self._h)
            self._h = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the hot path -------------------------------------------------------------------------
    def reserve(self, M):
        _lib.check(self._lib.naqs_ham_reserve(self._h, int(M)), "naqs_ham_reserve")

    def local_energy(self, keys, wf, kind="psi", row_begin=0, n_rows=None, out=None, weights=None, sums_out=None):
        """E_loc for table rows [row_begin, row_begin+n_rows) -> float64 tensor [n_rows, 2] (Re, Im).

        keys : int64 device tensor [M] (bit pattern of the uint64 keys), unique, physical
        wf   : device tensor [M, 2], float32/float64; (Re psi, Im psi) for kind="psi",
               (log|psi|, phase) for kind="log_psi"
        """
        M = keys.shape[0]
        if n_rows is None:
            n_rows = M - row_begin
        if wf.shape != (M, 2):
            raise ValueError(f"wave function must have shape [{M}, 2], got {tuple(wf.shape)}")
        if not (keys.is_cuda and wf.is_cuda and keys.dtype == torch.int64):
            raise ValueError("keys (int64) and wf must be device tensors")
        wf = wf.contiguous()
        keys = keys.contiguous()
        code = _KIND.get((kind, wf.dtype))
        if code is None:
            raise TypeError(f"unsupported wave-function kind/dtype: {kind}/{wf.dtype}")
        if out is None:
            out = torch.empty((n_rows, 2), dtype=torch.float64, device=self.device)
        if weights is not None:
            # fused: E_loc and (sum w Re E, sum w Im E, sum w Re(E)^2, sum w) of the produced rows in one launch
            w = weights.to(device=self.device, dtype=torch.float64).contiguous()
            if w.shape[0] != n_rows:
                raise ValueError("weights must cover exactly the produced rows")
            if sums_out is None:
                sums_out = torch.empty(4, dtype=torch.float64, device=self.device)
            st = self._lib.naqs_eloc_reduced(self._h, M, keys.data_ptr(), wf.data_ptr(), code, int(row_begin),
                                             int(n_rows), w.data_ptr(), out.data_ptr(), sums_out.data_ptr(),
                                             _stream_ptr(self.device))
            _lib.check(st, "naqs_eloc_reduced")
            return out, sums_out
        st = self._lib.naqs_eloc(self._h, M, keys.data_ptr(), wf.data_ptr(), code, int(row_begin), int(n_rows),
                                 out.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_eloc")
        return out

    def reduce(self, weights, eloc, out=None):
        """-> float64 device tensor [4] = (sum w Re E, sum w Im E, sum w Re(E)^2, sum w)."""
        w = weights.to(device=self.device, dtype=torch.float64).contiguous()
        if out is None:
            out = torch.empty(4, dtype=torch.float64, device=self.device)
        st = self._lib.naqs_eloc_reduce(self._h, eloc.shape[0], w.data_ptr(), eloc.contiguous().data_ptr(),
                                        out.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_eloc_reduce")
        return out

    # ---- connected states outside the table ----------------------------------------------------
    def n_offdiagonal_groups(self):
        return self.Kxy - (1 if self.diag_terms > 0 else 0)

    def sector_size(self):
        """Number of keys that pass the handle's particle-number filter (2^n without one)."""
        p = self.packed
        if p.n_alpha < 0:
            return 1 << p.n_qubits
        from math import comb
        return comb((p.n_qubits + 1) // 2, p.n_alpha) * comb(p.n_qubits // 2, p.n_beta)

    def connected_capacity(self, M, n_rows):
        """A capacity that ``connected_keys`` cannot overflow for ``n_rows`` rows of a table of ``M``: the smaller of
        rows x groups and what the sector has left (never more than the entry point's limit of 2^30)."""
        return max(0, min(n_rows * self.n_offdiagonal_groups(), self.sector_size() - M, 1 << 30))

    def connected_keys(self, keys, row_begin=0, n_rows=None, capacity=None):
        """The connected states of table rows [row_begin, row_begin + n_rows) that are not among ``keys``
        (``naqs_ham_connected``): key_i ^ xy_g over the rows and the non-diagonal groups, particle numbers conserved.

        -> (int64 device tensor, sorted ascending — or None when the set is larger than ``capacity`` —, count).
        On overflow ``count`` is only known to exceed ``capacity``.  The default capacity cannot overflow."""
        M = keys.shape[0]
        if n_rows is None:
            n_rows = M - row_begin
        if not (keys.is_cuda and keys.dtype == torch.int64):
            raise ValueError("keys must be an int64 device tensor")
        if row_begin < 0 or n_rows < 0 or row_begin + n_rows > M:
            raise ValueError(f"rows [{row_begin}, {row_begin + n_rows}) are not rows of a table of {M}")
        if capacity is None:
            capacity = self.connected_capacity(M, n_rows)
        capacity = int(capacity)
        if n_rows == 0:
            return torch.empty(0, dtype=torch.int64, device=self.device), 0
        keys = keys.contiguous()
        out = torch.empty(capacity, dtype=torch.int64, device=self.device)
        count = torch.empty(1, dtype=torch.int64, device=self.device)
        st = self._lib.naqs_ham_connected(self._h, M, keys.data_ptr(), int(row_begin), int(n_rows), capacity,
                                          out.data_ptr() if capacity > 0 else None, count.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_ham_connected")
        n = int(count.item())
        if n > capacity:
            return None, n
        # (bit patterns of uint64 keys: every supported key has bit 63 clear, so the signed order is the unsigned one)
        return torch.sort(out[:n]).values, n

    def exact_local_energy(self, net_handle, keys_buf, logpsi_buf, M, row_begin, n_rows, capacity, weights=None, out=None,
                           sums_out=None):
        """Exact local energies of table rows [row_begin, row_begin + n_rows) in one library call (``naqs_exact_eloc``):
        the connected states the table lacks are appended behind it in ``keys_buf``, ``net_handle``'s inference forward
        writes their log psi behind the table's in ``logpsi_buf``, and the E_loc kernel runs over the union.

        keys_buf   : int64 device tensor [>= M + capacity]; rows < M the table
        logpsi_buf : float32 device tensor [>= M + capacity, 2]; rows < M log psi of the table
        -> (E_loc float64 [n_rows, 2], sums float64 [4] or None, count, overflow).  On overflow (more than ``capacity``
        connected states; ``count`` is then a lower bound) nothing was evaluated and ``out`` / ``sums_out`` are untouched."""
        M, row_begin, n_rows, capacity = int(M), int(row_begin), int(n_rows), int(capacity)
        if not (keys_buf.is_cuda and keys_buf.dtype == torch.int64 and keys_buf.is_contiguous()):
            raise ValueError("keys_buf must be a contiguous int64 device tensor")
        if not (logpsi_buf.is_cuda and logpsi_buf.dtype == torch.float32 and logpsi_buf.is_contiguous()):
            raise ValueError("logpsi_buf must be a contiguous float32 device tensor")
        if capacity < 0 or keys_buf.shape[0] < M + capacity or tuple(logpsi_buf.shape[1:]) != (2,) or logpsi_buf.shape[0] < M + capacity:
            raise ValueError(f"buffers must hold the table and the capacity: {M} + {capacity} rows")
        if row_begin < 0 or n_rows < 0 or row_begin + n_rows > M:
            raise ValueError(f"rows [{row_begin}, {row_begin + n_rows}) are not rows of a table of {M}")
        if out is None:
            out = torch.empty((n_rows, 2), dtype=torch.float64, device=self.device)
        w_ptr = s_ptr = None
        if weights is not None:
            weights = weights.to(device=self.device, dtype=torch.float64).contiguous()
            if weights.shape[0] != n_rows:
                raise ValueError("weights must cover exactly the produced rows")
            if sums_out is None:
                sums_out = torch.empty(4, dtype=torch.float64, device=self.device)
            w_ptr, s_ptr = weights.data_ptr(), sums_out.data_ptr()
        info = (ctypes.c_int64 * 2)()
        st = self._lib.naqs_exact_eloc(net_handle, self._h, M, keys_buf.data_ptr(), logpsi_buf.data_ptr(), row_begin, n_rows,
                                       capacity, w_ptr, out.data_ptr(), s_ptr, info, _stream_ptr(self.device))
        _lib.check(st, "naqs_exact_eloc")
        return out, (sums_out if weights is not None else None), int(info[0]), bool(info[1])

    # ---- H restricted to the sampled states, matrix-free ----------------------------------------
    def matvec(self, keys, v, out=None):
        """out_i = sum_j H_ij v_j over the sampled keys (``naqs_hmatvec``).  v: real [M] or complex-as-pairs [M, 2]
        float64 device tensor; returns the same shape."""
        M = keys.shape[0]
        real = v.dim() == 1
        vv = torch.stack([v, torch.zeros_like(v)], -1) if real else v
        vv = vv.to(device=self.device, dtype=torch.float64).contiguous()
        res = torch.empty((M, 2), dtype=torch.float64, device=self.device) if out is None or real else out
        st = self._lib.naqs_hmatvec(self._h, M, keys.contiguous().data_ptr(), vv.data_ptr(), 0, M, res.data_ptr(),
                                    _stream_ptr(self.device))
        _lib.check(st, "naqs_hmatvec")
        return res[:, 0].contiguous() if real else res

    @torch.no_grad()
    def lowest_eigenpair(self, keys, max_iter=400, tol=1e-10, seed=0, v0=None, solver="lanczos", m_max=16, delta=1e-2):
        """Lowest eigenpair of H restricted to the sampled keys by Lanczos with full re-orthogonalisation, every
        product matrix-free on the device (no M x M or M x Kxy matrix is formed): the scalable form of the
        sampled-subspace diagonalisation of solve_H (energy.py:762-786).  -> (eigenvalue, eigenvector float64 [M]).
        ``v0``: a start vector [M] (normalised here) in place of the seeded random one; ``None`` is the random start, bit for
        bit.  ``last_lanczos_iterations`` holds the number of products the call took.

        ``solver="davidson"``: the diagonally preconditioned Davidson iteration of the library (``naqs_ham_eig_lowest``) from
        the same start — ``max_iter`` bounds its products, ``m_max`` (2..32) its basis, ``delta`` floors the preconditioner —
        and ``last_eig_info = dict(products, residual, status)`` (status 0 converged, 1 ``max_iter`` reached, 2 the basis spans
        the space, 3 breakdown).  H on the keys must be symmetric."""
        if solver not in ("lanczos", "davidson"):
            raise ValueError(f"solver must be 'lanczos' or 'davidson', got {solver!r}")
        M = keys.shape[0]
        if M == 0:
            raise ValueError("empty sample set")
        if solver == "davidson":
            return self._davidson(keys, int(max_iter), float(tol), seed, v0, int(m_max), float(delta))
        if v0 is None:
            gen = torch.Generator(device=self.device).manual_seed(int(seed))
            v = torch.randn(M, dtype=torch.float64, device=self.device, generator=gen)
        else:
            v = v0.to(device=self.device, dtype=torch.float64).clone()
            if v.shape != (M,) or not float(v.norm()) > 0:
                raise ValueError(f"v0 must be a non-zero vector of shape [{M}]")
        v /= v.norm()
        m_max = int(min(max_iter, M))
        V = torch.empty((m_max, M), dtype=torch.float64, device=self.device)
        from scipy.linalg import eigh_tridiagonal
        alpha, beta = [], []
        theta, s_vec, k = None, None, 0
        for k in range(m_max):
            V[k] = v
            w = self.matvec(keys, v)
            a = torch.dot(v, w)
            w = w - a * v - (beta[-1] * V[k - 1] if k > 0 else 0.0)
            for _ in range(2):                                   # full re-orthogonalisation, twice is enough
                w = w - V[:k + 1].t() @ (V[:k + 1] @ w)
            b = w.norm()
            a_h, b_h = torch.stack([a, b]).tolist()              # the iteration's one host synchronisation
            alpha.append(a_h)
            # lowest Ritz pair of the tridiagonal matrix only (O(k) bisection + inverse iteration, not a full eigh),
            # and not on every iteration once the basis is large: the test costs more than the product it saves
            last = k == m_max - 1 or b_h < 1e-14
            if k < 32 or k % 8 == 0 or last:
                if k == 0:
                    theta, s_vec = alpha[0], np.ones(1)
                else:
                    ev, evec = eigh_tridiagonal(np.array(alpha), np.array(beta), select="i", select_range=(0, 0))
                    theta, s_vec = float(ev[0]), evec[:, 0]
                resid = abs(b_h * s_vec[-1])
                if resid < tol * max(1.0, abs(theta)) or last:
                    break
            beta.append(b_h)
            v = w / b
        vec = torch.as_tensor(s_vec, dtype=torch.float64, device=self.device) @ V[:k + 1]
        vec = vec / vec.norm()
        self.last_lanczos_iterations = k + 1
        return float(theta), vec

    def _davidson(self, keys, max_iter, tol, seed, v0, m_max, delta):
        M = keys.shape[0]
        if not (keys.is_cuda and keys.dtype == torch.int64):
            raise ValueError("keys must be an int64 device tensor")
        if not 2 <= m_max <= 32:
            raise ValueError(f"m_max must lie in 2..32, got {m_max}")
        if max_iter < 1 or not (np.isfinite(tol) and tol > 0 and np.isfinite(delta) and delta > 0):
            raise ValueError("max_iter must be at least 1, tol and delta positive and finite")
        if v0 is None:
            gen = torch.Generator(device=self.device).manual_seed(int(seed))
            v = torch.randn(M, dtype=torch.float64, device=self.device, generator=gen)
        else:
            v = v0.to(device=self.device, dtype=torch.float64).contiguous()
            if v.shape != (M,):
                raise ValueError(f"v0 must be a non-zero vector of shape [{M}]")
        keys = keys.contiguous()
        vec = torch.empty(M, dtype=torch.float64, device=self.device)
        info = (ctypes.c_double * 4)()
        st = self._lib.naqs_ham_eig_lowest(self._h, M, keys.data_ptr(), v.data_ptr(), tol, max_iter, m_max, delta, vec.data_ptr(),
                                           info, _stream_ptr(self.device))
        if st == -1:                              # NAQS_ERR_INVALID: every other argument was checked above
            raise ValueError(f"v0 must be a non-zero finite vector of shape [{M}]")
        _lib.check(st, "naqs_ham_eig_lowest")
        self.last_lanczos_iterations = int(info[2])
        self.last_eig_info = dict(products=int(info[2]), residual=float(info[1]), status=int(info[3]))
        return float(info[0]), vec

    # ---- several vectors on one row walk; the k lowest roots -------------------------------------
    def block_product(self, keys, C):
        """``naqs_ham_block_product``: for the nb (1..8) rows of ``C`` [nb, M] (real float64) num[c, i] = sum_{j != i} H_ij C[c, j]
        over the table ``keys`` and diag[i] = H_ii, in ONE row walk — H C[c] = num[c] + diag * C[c].
        -> (num [nb, M], diag [M]) float64 device tensors."""
        M = keys.shape[0]
        if not (keys.is_cuda and keys.dtype == torch.int64):
            raise ValueError("keys must be an int64 device tensor")
        C = C.to(device=self.device, dtype=torch.float64).contiguous()
        if C.dim() != 2 or C.shape[1] != M or not 1 <= C.shape[0] <= 8:
            raise ValueError(f"C must have shape [1..8, {M}], got {tuple(C.shape)}")
        nb = C.shape[0]
        num = torch.empty((nb, M), dtype=torch.float64, device=self.device)
        diag = torch.empty(M, dtype=torch.float64, device=self.device)
        st = self._lib.naqs_ham_block_product(self._h, M, keys.contiguous().data_ptr(), nb, C.data_ptr(), num.data_ptr(), diag.data_ptr(),
                                              _stream_ptr(self.device))
        _lib.check(st, "naqs_ham_block_product")
        return num, diag

    @torch.no_grad()
    def lowest_eigenpairs(self, keys, k, max_iter=400, tol=1e-10, seed=0, v0=None, m_max=32, delta=1e-2):
        """The k' = min(k, M) lowest eigenpairs of H restricted to the sampled keys by the block Davidson iteration of the library
        (``naqs_ham_eig_lowest_k``: one block product per iteration).  1 <= k <= 8; ``max_iter`` bounds the products, ``m_max``
        (2 k .. 32) the basis, ``delta`` floors the preconditioner, as ``lowest_eigenpair(solver="davidson")``.  ``v0``: the starts
        [k, M]; ``None``: k draws of the seeded generator, row 0 the vector ``lowest_eigenpair`` draws.  H on the keys must be
        symmetric.  -> (theta float64 ndarray [k'] ascending, vecs float64 device tensor [k', M], rows of norm 1);
        ``last_eig_info = dict(products, residuals, status)`` (status as ``lowest_eigenpair``; 3: no correction was accepted)."""
        M = keys.shape[0]
        k, max_iter, m_max, tol, delta = int(k), int(max_iter), int(m_max), float(tol), float(delta)
        if M == 0:
            raise ValueError("empty sample set")
        if not 1 <= k <= 8:
            raise ValueError(f"k must lie in 1..8, got {k}")
        if not 2 * k <= m_max <= 32:
            raise ValueError(f"m_max must lie in 2 k..32 = {2 * k}..32, got {m_max}")
        if max_iter < 1 or not (np.isfinite(tol) and tol > 0 and np.isfinite(delta) and delta > 0):
            raise ValueError("max_iter must be at least 1, tol and delta positive and finite")
        if not (keys.is_cuda and keys.dtype == torch.int64):
            raise ValueError("keys must be an int64 device tensor")
        kk = min(k, M)
        if v0 is None:
            gen = torch.Generator(device=self.device).manual_seed(int(seed))
            v = torch.stack([torch.randn(M, dtype=torch.float64, device=self.device, generator=gen) for _ in range(k)])
        else:
            v = v0.to(device=self.device, dtype=torch.float64).contiguous()
            if v.shape != (k, M):
                raise ValueError(f"v0 must have shape [{k}, {M}], got {tuple(v.shape)}")
        keys = keys.contiguous()
        vecs = torch.empty((kk, M), dtype=torch.float64, device=self.device)
        theta, rho, info = (ctypes.c_double * kk)(), (ctypes.c_double * kk)(), (ctypes.c_int32 * 2)()
        st = self._lib.naqs_ham_eig_lowest_k(self._h, M, keys.data_ptr(), k, v.data_ptr(), tol, max_iter, m_max, delta, vecs.data_ptr(),
                                             theta, rho, info, _stream_ptr(self.device))
        if st == -1:                              # NAQS_ERR_INVALID: every other argument was checked above
            raise ValueError(f"v0 must hold {kk} finite, linearly independent rows of shape [{M}]")
        _lib.check(st, "naqs_ham_eig_lowest_k")
        self.last_lanczos_iterations = int(info[0])
        self.last_eig_info = dict(products=int(info[0]), residuals=[float(r) for r in rho], status=int(info[1]))
        return np.array(list(theta), np.float64), vecs

    # ---- Epstein-Nesbet second-order correction of a subspace energy -----------------------------
    def pt2(self, keys, c, e0, ext_keys, rows=False):
        """``naqs_ham_pt2``: for every row key a of ``ext_keys`` num_a = sum_j H_aj c_j over the table ``keys`` (off-diagonal
        groups only) and diag_a = H_aa, and the four sums with den_a = e0 - diag_a:
        (sum_{den<0} num^2 / den, sum_{den<0} num^2, rows with den >= 0, sum of num^2 over those rows).

        keys, ext_keys : int64 device tensors; c : real float64 device tensor [M]
        -> float64 device tensor [4]; with ``rows=True`` (out4, num [n_ext], diag [n_ext])."""
        M, n_ext = keys.shape[0], ext_keys.shape[0]
        if not (keys.is_cuda and ext_keys.is_cuda and keys.dtype == torch.int64 and ext_keys.dtype == torch.int64):
            raise ValueError("keys and ext_keys must be int64 device tensors")
        c = c.to(device=self.device, dtype=torch.float64).contiguous()
        if c.shape != (M,):
            raise ValueError(f"c must have shape [{M}], got {tuple(c.shape)}")
        keys, ext_keys = keys.contiguous(), ext_keys.contiguous()
        out4 = torch.empty(4, dtype=torch.float64, device=self.device)
        num = torch.empty(n_ext, dtype=torch.float64, device=self.device) if rows else None
        diag = torch.empty(n_ext, dtype=torch.float64, device=self.device) if rows else None
        st = self._lib.naqs_ham_pt2(self._h, M, keys.data_ptr(), c.data_ptr(), float(e0), n_ext,
                                    ext_keys.data_ptr() if n_ext else None, num.data_ptr() if rows and n_ext else None,
                                    diag.data_ptr() if rows and n_ext else None, out4.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_ham_pt2")
        return (out4, num, diag) if rows else out4

    @torch.no_grad()
    def pt2_correction(self, keys, vec, e0=None, max_external=1 << 27):
        """Second-order Epstein-Nesbet correction of the energy of ``vec`` in the subspace ``keys``:
        E_PT2 = sum_a (sum_j H_aj vec_j)^2 / (e0 - H_aa) over the states a outside ``keys`` that one Hamiltonian term connects
        to it (``connected_keys``).  ``e0=None``: the Rayleigh quotient of ``vec``.  An external state with H_aa >= e0 (an
        intruder) is left out of the sum and counted.  The external set is held whole, 8 bytes a key: a set whose capacity
        exceeds ``max_external`` keys raises ValueError.

        -> dict(e0, e_pt2, n_external, n_intruders, residual2, intruder_residual2)"""
        M = keys.shape[0]
        vec = vec.to(device=self.device, dtype=torch.float64).contiguous()
        if e0 is None:
            e0 = float(torch.dot(vec, self.matvec(keys, vec)) / torch.dot(vec, vec))
        capacity = self.connected_capacity(M, M)
        if capacity > max_external:
            raise ValueError(f"the connected set of {M} keys may hold {capacity} keys, more than max_external = {max_external}")
        ext, n_ext = self.connected_keys(keys, capacity=capacity)
        out4 = self.pt2(keys, vec, e0, ext).tolist()
        return dict(e0=float(e0), e_pt2=out4[0], n_external=int(n_ext), n_intruders=int(out4[2]), residual2=out4[1],
                    intruder_residual2=out4[3])

    # ---- selected CI: the subspace grown by PT2 importance ------------------------------------------
    # tie_rtol's default: on the committed fixtures symmetry partners (spin flip, spatial) have importances equal to <= 1e-13
    # relative — rounding noise — while the smallest genuine gap met at a cut was 1.8e-4 relative; 1e-9 sits four orders above
    # the one and five below the other, so a cut never orders partners by noise and never merges distinct groups.
    def pt2_select(self, ext_keys, num, diag, e0, k, eps_min=0.0, tie_rtol=1e-9):
        """``naqs_ham_pt2_select`` on the rows ``pt2(rows=True)`` returns: eps_a = num_a^2 / (diag_a - e0) (+inf for an intruder:
        not diag_a - e0 > 0, or num_a NaN); eligible: eps > 0 and eps >= eps_min; with tau the k-th largest eligible eps, every
        eligible row with eps >= tau (1 - tie_rtol) is selected — all eligible rows when k reaches their number, none when
        k <= 0.  A near-degenerate group at the cut is taken whole, so the count may exceed k.

        -> (selected keys in row order, int64 device tensor; number of intruders among them).  One read-back (the counts)."""
        n_ext = ext_keys.shape[0]
        if not (ext_keys.is_cuda and ext_keys.dtype == torch.int64):
            raise ValueError("ext_keys must be an int64 device tensor")
        num = num.to(device=self.device, dtype=torch.float64).contiguous()
        diag = diag.to(device=self.device, dtype=torch.float64).contiguous()
        if num.shape != (n_ext,) or diag.shape != (n_ext,):
            raise ValueError(f"num and diag must have shape [{n_ext}]")
        ext_keys = ext_keys.contiguous()
        out = torch.empty(n_ext, dtype=torch.int64, device=self.device)
        count = torch.empty(2, dtype=torch.int64, device=self.device)
        st = self._lib.naqs_ham_pt2_select(self._h, n_ext, ext_keys.data_ptr() if n_ext else None, num.data_ptr() if n_ext else None,
                                           diag.data_ptr() if n_ext else None, float(e0), int(k), float(eps_min), float(tie_rtol),
                                           n_ext, out.data_ptr() if n_ext else None, count.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_ham_pt2_select")
        n_sel, n_intr = count.tolist()
        return out[:n_sel], int(n_intr)

    @torch.no_grad()
    def selected_ci(self, keys, n_add, eps_min=0.0, tie_rtol=1e-9, max_states=1 << 20, max_external=1 << 27, tol=1e-10,
                    solver="lanczos"):
        """Selected CI from the subspace ``keys`` (int64 device tensor, unique): diagonalise, measure every connected state's
        second-order importance, move the most important ones into the subspace, diagonalise again.

        ``n_add``: a sequence of ints — k of each growth step, so len(n_add) + 1 iterations — or ``(n_iter, grow)`` with a
        float ``grow``: n_iter iterations, k = ceil(grow M) at each growth step.  Iteration t: Lanczos on S_t (the first from
        lowest_eigenpair's own random start, as solve_H; later ones from (c_{t-1}, 0)), ``connected_keys``, ``pt2(rows=True)``,
        the record, and — unless it is the last — ``pt2_select`` and S_{t+1} = cat(S_t, selected).  Every E_S is variational
        and the subspaces are nested, so E_S never rises; E_S + E_PT2 is not variational.

        ``solver``: lowest_eigenpair's ("lanczos" or "davidson"), for every iteration.

        -> dict(keys, vec, history=[dict(M, e0, e_pt2, n_external, n_intruders, n_added)], stopped, extrapolated);
        ``stopped``: "schedule" (all iterations done), "connected set empty", "nothing eligible" or "max_states"."""
        ks, grow = _sci_schedule(n_add)
        n_iter = len(ks) + 1 if grow is None else ks
        keys = keys.contiguous()
        history, vec, stopped = [], None, "schedule"
        for t in range(n_iter):
            M = keys.shape[0]
            e0, vec = self.lowest_eigenpair(keys, tol=tol, v0=vec, solver=solver)
            capacity = self.connected_capacity(M, M)
            if capacity > max_external:
                raise ValueError(f"the connected set of {M} keys may hold {capacity} keys, more than max_external = {max_external}")
            ext, n_ext = self.connected_keys(keys, capacity=capacity)
            out4, num, diag = self.pt2(keys, vec, e0, ext, rows=True)
            out4 = out4.tolist()
            rec = dict(M=M, e0=float(e0), e_pt2=out4[0], n_external=int(n_ext), n_intruders=int(out4[2]), n_added=0)
            history.append(rec)
            if n_ext == 0:
                stopped = "connected set empty"
                break
            if t == n_iter - 1:
                break
            k = int(ks[t]) if grow is None else int(np.ceil(grow * M))
            sel, _ = self.pt2_select(ext, num, diag, e0, k, eps_min=eps_min, tie_rtol=tie_rtol)
            if sel.shape[0] == 0:
                stopped = "nothing eligible"
                break
            if M + sel.shape[0] > max_states:
                stopped = "max_states"
                break
            rec["n_added"] = int(sel.shape[0])
            keys = torch.cat([keys, sel])
            vec = torch.cat([vec, torch.zeros(sel.shape[0], dtype=torch.float64, device=self.device)])
        return dict(keys=keys, vec=vec, history=history, stopped=stopped, extrapolated=extrapolate_pt2(history))

    # ---- selected CI for several roots: one walk over the external rows, a state-averaged importance ----
    def pt2_block(self, keys, C, e, ext_keys, rows=False):
        """``naqs_ham_pt2_block``: ``pt2`` for the nb (1..8) rows of ``C`` [nb, M] with the energies ``e`` [nb], in ONE walk over
        ``ext_keys`` — row c of every output has the bits ``pt2(keys, C[c], e[c], ext_keys)`` gives.
        -> out4 float64 device tensor [nb, 4]; with ``rows=True`` (out4, num [nb, n_ext], diag [n_ext])."""
        M, n_ext = keys.shape[0], ext_keys.shape[0]
        if not (keys.is_cuda and ext_keys.is_cuda and keys.dtype == torch.int64 and ext_keys.dtype == torch.int64):
            raise ValueError("keys and ext_keys must be int64 device tensors")
        C = C.to(device=self.device, dtype=torch.float64).contiguous()
        if C.dim() != 2 or C.shape[1] != M or not 1 <= C.shape[0] <= 8:
            raise ValueError(f"C must have shape [1..8, {M}], got {tuple(C.shape)}")
        nb = C.shape[0]
        e = np.asarray(e, np.float64).reshape(-1)
        if e.shape != (nb,) or not np.all(np.isfinite(e)):
            raise ValueError(f"e must hold {nb} finite energies")
        keys, ext_keys = keys.contiguous(), ext_keys.contiguous()
        out4 = torch.empty((nb, 4), dtype=torch.float64, device=self.device)
        num = torch.empty((nb, n_ext), dtype=torch.float64, device=self.device) if rows else None
        diag = torch.empty(n_ext, dtype=torch.float64, device=self.device) if rows else None
        st = self._lib.naqs_ham_pt2_block(self._h, M, keys.data_ptr(), nb, C.data_ptr(), (ctypes.c_double * nb)(*e.tolist()), n_ext,
                                          ext_keys.data_ptr() if n_ext else None, num.data_ptr() if rows and n_ext else None,
                                          diag.data_ptr() if rows and n_ext else None, out4.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_ham_pt2_block")
        return (out4, num, diag) if rows else out4

    def pt2_select_roots(self, ext_keys, num, diag, e, k, weights=None, eps_min=0.0, tie_rtol=1e-9):
        """``naqs_ham_pt2_select_avg`` on the rows ``pt2_block(rows=True)`` returns: ``pt2_select`` with the importance
        eps_a = sum_j w_j num_ja^2 / (diag_a - e_j) over the roots of non-zero weight, in order (+inf when a is an intruder of
        any of them).  ``weights=None``: 1 / nb each; a weight of 0 takes its root out of the rule altogether.

        -> (selected keys in row order, int64 device tensor; number of intruders among them).  One read-back (the counts)."""
        n_ext = ext_keys.shape[0]
        if not (ext_keys.is_cuda and ext_keys.dtype == torch.int64):
            raise ValueError("ext_keys must be an int64 device tensor")
        num = num.to(device=self.device, dtype=torch.float64).contiguous()
        diag = diag.to(device=self.device, dtype=torch.float64).contiguous()
        if num.dim() != 2 or not 1 <= num.shape[0] <= 8 or num.shape[1] != n_ext or diag.shape != (n_ext,):
            raise ValueError(f"num must have shape [1..8, {n_ext}] and diag [{n_ext}]")
        nb = num.shape[0]
        e = np.asarray(e, np.float64).reshape(-1)
        w = np.full(nb, 1.0 / nb) if weights is None else np.asarray(weights, np.float64).reshape(-1)
        if e.shape != (nb,) or w.shape != (nb,):
            raise ValueError(f"e and weights must hold {nb} entries each")
        if not np.all(np.isfinite(w) & (w >= 0)) or not np.any(w > 0):
            raise ValueError("weights must be finite and non-negative, at least one of them positive")
        if not np.all(np.isfinite(e[w > 0])):
            raise ValueError("the energy of every root of non-zero weight must be finite")
        ext_keys = ext_keys.contiguous()
        out = torch.empty(n_ext, dtype=torch.int64, device=self.device)
        count = torch.empty(2, dtype=torch.int64, device=self.device)
        st = self._lib.naqs_ham_pt2_select_avg(self._h, n_ext, ext_keys.data_ptr() if n_ext else None, nb, num.data_ptr() if n_ext else None,
                                               diag.data_ptr() if n_ext else None, (ctypes.c_double * nb)(*e.tolist()),
                                               (ctypes.c_double * nb)(*w.tolist()), int(k), float(eps_min), float(tie_rtol), n_ext,
                                               out.data_ptr() if n_ext else None, count.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_ham_pt2_select_avg")
        n_sel, n_intr = count.tolist()
        return out[:n_sel], int(n_intr)

    @torch.no_grad()
    def selected_ci_roots(self, keys, n_roots, n_add, weights=None, eps_min=0.0, tie_rtol=1e-9, max_states=1 << 20,
                          max_external=1 << 27, tol=1e-10):
        """``selected_ci`` for the ``n_roots`` (1..8) lowest states at once, the subspace grown by their averaged importance.
        Iteration t: ``lowest_eigenpairs(keys, n_roots, tol=tol)`` (the first from the solver's own start, later ones from the
        previous vectors padded with zeros, which stay orthonormal), ``connected_keys``, ONE ``pt2_block(rows=True)`` for all
        roots, the record, and — unless it is the last — ``pt2_select_roots`` and S_{t+1} = cat(S_t, selected).  The roots are
        the n_roots lowest of each subspace, ascending; none is followed from one iteration to the next.  ``n_add`` as
        ``selected_ci``; fewer keys than roots: ValueError; ``max_external`` bounds n_roots times the connected set's capacity.

        -> dict(keys, eigs, vecs, history=[dict(M, e0=[..], e_pt2=[..], n_external, n_intruders=[..], n_added)], stopped,
        extrapolated=[per root, extrapolate_pt2 on its (e0, e_pt2) series]); ``stopped`` as ``selected_ci``."""
        n_roots = int(n_roots)
        if not 1 <= n_roots <= 8:
            raise ValueError(f"n_roots must lie in 1..8, got {n_roots}")
        if keys.shape[0] < n_roots:
            raise ValueError(f"{keys.shape[0]} keys cannot carry {n_roots} roots")
        ks, grow = _sci_schedule(n_add)
        n_iter = len(ks) + 1 if grow is None else ks
        keys = keys.contiguous()
        history, eigs, vecs, stopped = [], None, None, "schedule"
        for t in range(n_iter):
            M = keys.shape[0]
            eigs, vecs = self.lowest_eigenpairs(keys, n_roots, tol=tol, v0=vecs)
            capacity = self.connected_capacity(M, M)
            if n_roots * capacity > max_external:
                raise ValueError(f"the connected set of {M} keys may hold {capacity} keys for each of {n_roots} roots, more than "
                                 f"max_external = {max_external}")
            ext, n_ext = self.connected_keys(keys, capacity=capacity)
            out4, num, diag = self.pt2_block(keys, vecs, eigs, ext, rows=True)
            out4 = out4.tolist()
            rec = dict(M=M, e0=[float(x) for x in eigs], e_pt2=[r[0] for r in out4], n_external=int(n_ext),
                       n_intruders=[int(r[2]) for r in out4], n_added=0)
            history.append(rec)
            if n_ext == 0:
                stopped = "connected set empty"
                break
            if t == n_iter - 1:
                break
            k = int(ks[t]) if grow is None else int(np.ceil(grow * M))
            sel, _ = self.pt2_select_roots(ext, num, diag, eigs, k, weights=weights, eps_min=eps_min, tie_rtol=tie_rtol)
            if sel.shape[0] == 0:
                stopped = "nothing eligible"
                break
            if M + sel.shape[0] > max_states:
                stopped = "max_states"
                break
            rec["n_added"] = int(sel.shape[0])
            keys = torch.cat([keys, sel])
            vecs = torch.cat([vecs, torch.zeros((n_roots, sel.shape[0]), dtype=torch.float64, device=self.device)], dim=1)
        per_root = [[dict(e0=h["e0"][j], e_pt2=h["e_pt2"][j]) for h in history] for j in range(n_roots)]
        return dict(keys=keys, eigs=[float(x) for x in eigs], vecs=vecs, history=history, stopped=stopped,
                    extrapolated=[extrapolate_pt2(series) for series in per_root])

    # ---- inner ring ----------------------------------------------------------------------------
    def dense_hij(self, keys):
        """Device counterpart of get_Hij_cy: float64 [M, Kxy], H[i, key_i ^ xy_g]."""
        M = keys.shape[0]
        out = torch.empty((M, self.Kxy), dtype=torch.float64, device=self.device)
        st = self._lib.naqs_get_hij(self._h, M, keys.contiguous().data_ptr(), out.data_ptr(),
                                    _stream_ptr(self.device))
        _lib.check(st, "naqs_get_hij")
        return out

    # ---- measurement ---------------------------------------------------------------------------
    def prof_enable(self, max_records, stride=1):
        _lib.check(self._lib.naqs_prof_enable(self._h, int(max_records)), "naqs_prof_enable")
        _lib.check(self._lib.naqs_prof_stride(self._h, int(stride)), "naqs_prof_stride")

    def prof_read(self):
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        _lib.check(self._lib.naqs_prof_read(self._h, ctypes.byref(ms), ctypes.byref(n)), "naqs_prof_read")
        return ms.value, n.value

    def last_kernel(self):
        """Name (with template arguments) of the kernel the most recent call launched (measurement aid)."""
        buf = ctypes.create_string_buffer(128)
        _lib.check(self._lib.naqs_ham_last_kernel(self._h, buf, 128), "naqs_ham_last_kernel")
        return buf.value.decode()

    def closed_counts(self):
        """(class D groups, class S groups, class L groups, table bytes) of the default kernel's view of this handle."""
        out = (ctypes.c_int64 * 4)()
        _lib.check(self._lib.naqs_ham_closed_counts(self._h, ctypes.byref(out)), "naqs_ham_closed_counts")
        return tuple(int(v) for v in out)


def popcount_parity_device(arr):
    """Device counterpart of src.utils.hamiltonian_math.popcount_parity: int8 tensor, same shape.
    Raises TypeError on unsupported dtypes like the reference (hamiltonian_math.pyx:484)."""
    if arr.dtype not in (torch.int16, torch.int32, torch.int64):
        raise TypeError(f"Unsupported array dtype for popcount_parity(...): {arr.dtype}.")
    lib = _lib.load_library()
    a = arr.contiguous()
    out = torch.empty(a.shape if a.dim() > 1 else (a.numel(), 1), dtype=torch.int8, device=a.device)
    st = lib.naqs_popcount_parity(a.data_ptr(), a.element_size(), a.numel(), out.data_ptr(), _stream_ptr(a.device))
    _lib.check(st, "naqs_popcount_parity")
    return out


def csr_mv_device(data, indices, indptr, v):
    """Device counterpart of src.utils.sparse_math.sparse_dense_mv (f64 CSR x complex128 [n,2])."""
    lib = _lib.load_library()
    rows = indptr.numel() - 1
    out = torch.empty((rows, 2), dtype=torch.float64, device=v.device)
    st = lib.naqs_csr_mv(rows, data.contiguous().data_ptr(), indices.contiguous().data_ptr(),
                         indptr.contiguous().data_ptr(), v.contiguous().data_ptr(), out.data_ptr(),
                         _stream_ptr(v.device))
    _lib.check(st, "naqs_csr_mv")
    return out


class PauliHamiltonian:
    """Factory with the reference's signature (hamiltonian.py:47-61)."""

    @staticmethod
    def get(hilbert, qubit_hamiltonian, hamiltonian_fname=None, restricted_idxs=None,
            n_excitations_max=None, verbose=False, dtype=np.float64, device=None):
        if isinstance(qubit_hamiltonian, PackedHamiltonian):
            packed = qubit_hamiltonian
        else:
            packed = pack_qubit_hamiltonian(qubit_hamiltonian.terms, hilbert.N, hilbert.N_alpha, hilbert.N_beta,
                                            n_excitations_max=n_excitations_max, n_occ=getattr(hilbert, "N_occ", 0))
        return MatrixFreePauliHamiltonian(hilbert, packed, verbose=verbose, device=device)


class MatrixFreePauliHamiltonian(DevicePauliHamiltonian):
    """``_PauliHamiltonianDynamic`` counterpart: same method names, nothing cached."""

    def __init__(self, hilbert, packed, verbose=False, device=None):
        super().__init__(packed, device=device)
        self.hilbert = hilbert
        self.verbose = verbose
        self._frozen_H = False

    def update_H(self, state_idx=None, check_unseen=True, assume_unique=False):
        return None          # matrix elements are regenerated per call; there is no cache to update

    def freeze_H(self):
        self._frozen_H = True

    def unfreeze_H(self):
        self._frozen_H = False

    def is_frozen(self):
        return self._frozen_H

    def get_H(self, idxs):
        """H restricted to the given states as a scipy CSR in *sample order* (hamiltonian.py:93-111,
        without the full-sample reordering quirk Q1).  Diagnostic path (solve_H); builds on
        ``naqs_get_hij`` and keeps explicit zeros like the reference."""
        from scipy.sparse import csr_matrix
        keys = keys_to_device(idxs, self.device)
        hij = self.dense_hij(keys).cpu().numpy()
        k = keys.cpu().numpy().view(np.uint64)
        xy_g = np.unique(self.packed.xy)
        order = np.argsort(k, kind="stable")
        ks = k[order]
        j = k[:, None] ^ xy_g[None, :]
        pos = np.searchsorted(ks, j)
        pos[pos == len(ks)] = 0
        hit = ks[pos] == j
        rows = np.broadcast_to(np.arange(len(k))[:, None], j.shape)[hit]
        cols = order[pos[hit]]
        return csr_matrix((hij[hit], (rows, cols)), shape=(len(k), len(k)))


def _sci_schedule(n_add):
    """``selected_ci``'s n_add -> (list of k, None) or (n_iter, grow)."""
    n_add = tuple(n_add)
    if len(n_add) == 2 and isinstance(n_add[1], float):
        n_iter, grow = int(n_add[0]), float(n_add[1])
        if n_iter < 1 or not grow > 0:
            raise ValueError(f"n_add = (n_iter, grow) needs n_iter >= 1 and grow > 0, got {n_add}")
        return n_iter, grow
    if any(int(k) != k for k in n_add):
        raise ValueError(f"n_add must be a sequence of ints or (n_iter, grow) with a float grow, got {n_add}")
    return [int(k) for k in n_add], None


def extrapolate_pt2(history, n_fit=3):
    """The intercept at E_PT2 = 0 of the least-squares line of e0 against e_pt2 over the last ``n_fit`` (>= 3) iterations of
    ``selected_ci`` with e_pt2 < 0; None with fewer than three of them.  Not variational."""
    pts = [(h["e_pt2"], h["e0"]) for h in history if h["e_pt2"] < 0][-max(3, int(n_fit)):]
    if len(pts) < 3:
        return None
    x, y = np.array(pts).T
    return float(np.polyfit(x, y, 1)[1])
