/*
 * naqs_hip.h — C ABI of libnaqs_hip.so: the MI355X (gfx950) local-energy path of a
 * neural-autoregressive-quantum-state VMC step.
 *
 * The reference (tomdbar/naqs-for-quantum-chemistry) has no C ABI of its own; its native seam is
 * three Cython extension modules that its Python imports.  Every entry
 * point below names the reference interface it replaces (file:line relative to the reference
 * repository).  INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross the boundary;
 *   - every function returns NAQS_OK (0) or a negative naqs_status; nothing throws;
 *   - `*_dev` pointers are device memory on the handle's device and stay owned by the caller;
 *   - all device work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the null
 *     stream) and is asynchronous: results are valid after the stream is synchronised;
 *   - a handle is bound to one device, owns its packed term tables and scratch buffers, and must
 *     not be used from two streams/threads at the same time;
 *   - bit-string convention: qubit q <-> bit q of the key; even bits = alpha spin-orbitals, odd
 *     bits = beta (src/utils/hilbert.py:446-449, :573-581).
 */
#ifndef NAQS_HIP_H
#define NAQS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NAQS_ABI_VERSION 9

typedef struct naqs_ham naqs_ham_t;

enum naqs_status {
    NAQS_OK = 0,
    NAQS_ERR_INVALID = -1,      /* bad argument (NULL pointer, negative size, range outside table) */
    NAQS_ERR_HIP = -2,          /* a HIP runtime call failed; see naqs_last_hip_error() */
    NAQS_ERR_NOMEM = -3,        /* host or device allocation failed */
    NAQS_ERR_UNSUPPORTED = -4,  /* e.g. n_qubits > 64, unsupported element width */
    NAQS_ERR_NO_DEVICE = -5     /* no usable HIP device / wrong architecture */
};

/* How the wave function of the sampled states is handed over (second index: 2 components). */
enum naqs_psi_kind {
    NAQS_PSI_F32 = 0,     /* float  [M][2] = (Re psi, Im psi): what the reference passes, energy.py:241-243 */
    NAQS_PSI_F64 = 1,     /* double [M][2] = (Re psi, Im psi) */
    NAQS_LOGPSI_F32 = 2,  /* float  [M][2] = (log|psi|, phase): network output, wavefunction.py:167-183 */
    NAQS_LOGPSI_F64 = 3   /* double [M][2] = (log|psi|, phase) */
};

int naqs_abi_version(void);
/* 16 hex digits: SHA-256 prefix of the kernel sources (the .hip and .hpp files under csrc) this library was built from.  No counterpart in
 * the reference; it lets measurement tooling (bench.py, tools/collect_pmc.py) tie replayed hardware-counter files to the
 * exact kernels they were collected on. */
const char *naqs_source_hash(void);
const char *naqs_strerror(int status);
/* hipError_t of the most recent failing HIP call on this thread (0 if none) and its text.  When the failure was a
 * device-side wait that ran out of its budget (naqs_device_check below), the text names the kernel site, the waiting
 * workgroup and the index it waited for. */
int naqs_last_hip_error(void);
const char *naqs_last_hip_error_string(void);
/* Kernels of this library that wait for a word another workgroup publishes (sampler look-back, column-split log-psi
 * tiles, fused sums, re-pack scale chain) give up after NAQS_POLL_BUDGET_MS (default 2000) instead of hanging: the wave
 * records the site in the error word of the network handle that launched the kernel (ABI 8; one word per device before: two
 * runs sharing a GPU could take each other's failures) and leaves without writing results.  Every entry point of a handle
 * looks at the handle's word when it is called; this call looks at the words of ALL live handles of the device on demand
 * (e.g. after a stream synchronisation) and reports the first it finds: NAQS_OK, or NAQS_ERR_HIP with
 * naqs_last_hip_error_string() describing the wait.  The reference has no counterpart (its only failure path in the loop is
 * MaxBatchSizeExceededError, src/naqs/network/nade.py:39-40, 710-712 -> src/optimizer/energy.py:939-946); a hang has to
 * become an error somewhere. */
int naqs_device_check(int device);

/* Number of HIP devices visible to the library (0 when there is none); never fails. */
int naqs_device_count(void);

/*
 * Host-only: group K Pauli terms by their XY (bit-flip) mask — the dedupe of
 * src/optimizer/hamiltonian.py:248-252 (np.unique(XY, return_inverse)) turned into a CSR:
 *   xy_g[Kxy] ascending unique masks, row_ptr[Kxy+1], and per-term yz_t[K], c_t[K], order[K]
 *   (order[t] = original term index; terms keep ascending original order inside a group, so a
 *   sequential sum over a group reproduces the reference's summation order, hamiltonian_math.pyx:95-98).
 * Output arrays are caller-allocated with room for K (row_ptr: K+1) entries.
 */
int naqs_terms_group(int64_t K, const uint64_t *xy, const uint64_t *yz, const double *coeff,
                     int64_t *Kxy_out, uint64_t *xy_g, int32_t *row_ptr,
                     uint64_t *yz_t, double *c_t, int64_t *order);

/*
 * Create a device-resident Pauli Hamiltonian from K pre-processed terms
 *   xy[k]   bit q set iff the Pauli on qubit q is X or Y      (hamiltonian.py:389-390)
 *   yz[k]   bit q set iff the Pauli on qubit q is Y or Z      (hamiltonian.py:391-393, :402-403)
 *   coeff[k] = Re(i^{nY}) * coefficient, real                 (hamiltonian.py:416, :424)
 * host arrays, copied.  Replaces _PauliHamiltonianDynamic.__init__ (hamiltonian.py:241-262); the
 * lazily cached scipy CSR matrix of the reference (hamiltonian.py:86, :350-363) has no counterpart:
 * matrix elements are regenerated on the fly.
 * n_alpha / n_beta: electrons per spin (particle-number filter, replaces the 2^N look-up table of
 * src/utils/hilbert.py:429-434); pass -1/-1 for an unrestricted space.
 */
int naqs_ham_create(int n_qubits, int n_alpha, int n_beta, int64_t K,
                    const uint64_t *xy, const uint64_t *yz, const double *coeff,
                    int device, naqs_ham_t **out);
int naqs_ham_destroy(naqs_ham_t *h);

/* info[0..7] = { K, Kxy, n_qubits, n_alpha, n_beta, key_bits (32|64), diag_terms, device } */
int naqs_ham_info(const naqs_ham_t *h, int64_t info[8]);

/* Pre-size the scratch buffers for up to M sampled states (otherwise grown on demand, which
 * synchronises the device). */
int naqs_ham_reserve(naqs_ham_t *h, int64_t M);

/*
 * Local energies.  Replaces OptimizerBase.calculate_local_energy (src/optimizer/energy.py:219-263)
 * = update_H (hamiltonian.py:272-370: get_Hij_cy + popcount_parity) + get_H (hamiltonian.py:93-111)
 * + sparse_dense_mv (sparse_math.pyx:47-100), fused and matrix-free:
 *
 *   E_loc[i] = conj( sum_j H[i,j] psi[j] / psi[i] ),  j restricted to the M sampled states
 *   H[i, key_i ^ xy_g] = sum_{k in g} coeff_k (-1)^{popcount(key_i & yz_k)}
 *
 * keys_dev[M]   unique sampled bit-strings (any order), all physical
 * psi_dev       per psi_kind, [M][2]
 * rows          E_loc is produced for table rows [row_begin, row_begin + n_rows) only — the shard of
 *               one rank; couplings are still looked up in the whole table
 * eloc_dev      double [n_rows][2] = (Re, Im)
 */
int naqs_eloc(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, const void *psi_dev, int psi_kind,
              int64_t row_begin, int64_t n_rows, double *eloc_dev, void *stream);

/*
 * naqs_eloc followed by naqs_eloc_reduce over the produced rows, enqueued by one call:
 * w_dev[n_rows] are the weights of the produced rows, out4_dev as below.
 */
int naqs_eloc_reduced(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, const void *psi_dev, int psi_kind,
                      int64_t row_begin, int64_t n_rows, const double *w_dev, double *eloc_dev,
                      double *out4_dev, void *stream);

/*
 * Weighted sums over n local energies, deterministic order:
 *   out4_dev = { sum w Re(E), sum w Im(E), sum w Re(E)^2, sum w }
 * from which <E> and Var follow as in _SGD_step (src/optimizer/energy.py:367-377).
 */
int naqs_eloc_reduce(naqs_ham_t *h, int64_t n, const double *w_dev, const double *eloc_dev,
                     double *out4_dev, void *stream);

/*
 * Matrix-free product with the Hamiltonian restricted to the sampled states: out_i = sum_j H_ij v_j over the M keys
 * (complex float64 [M][2] in and out; H is real symmetric).  The mat-vec of get_H(idxs) (src/optimizer/hamiltonian.py:93-111)
 * without materialising the sub-matrix — what the sampled-subspace diagonalisation of solve_H (src/optimizer/energy.py:762-786)
 * needs once the sample set is too large for a dense M x Kxy table.  Same kernel and row sharding as naqs_eloc.
 */
int naqs_hmatvec(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, const double *v_dev, int64_t row_begin,
                 int64_t n_rows, double *out_dev, void *stream);

/*
 * The connected states of table rows [row_begin, row_begin + n_rows) that the table does not hold: what the reference's
 * calculate_local_energy(set_unsampled_states_to_zero=False) would need psi for and never computes — its branch is
 * `raise NotImplementedError()` above a commented-out sketch (src/optimizer/energy.py:227-235, 250-258).  The output is
 * the set of keys j = key_i ^ xy_g over the rows i of the range and every non-diagonal XY group g of the handle
 * (xy_g != 0) such that j passes the handle's particle-number filter (every j does when n_alpha = n_beta = -1) and j is
 * not among the M keys; each j once, in any order; whether H_ij happens to sum to zero does not enter.
 *
 * out_keys_dev[capacity]  the set; *count_dev its size.  When the set is larger than `capacity` the call still
 *                         returns NAQS_OK, with *count_dev > capacity (a lower bound of the size, not the size) and
 *                         unspecified out_keys_dev contents; nothing is written past `capacity` and the call takes no
 *                         longer than a successful one.  capacity = 0 (out_keys_dev may be null) asks "is the set empty".
 * With E_loc over the table keys + set, rows [row_begin, row_begin + n_rows), this gives the local energy over ALL
 * connected states.  The call rebuilds the handle's sample-key table (like naqs_eloc) and owns a scratch set of
 * >= 2 capacity 64-bit slots that grows on demand.  n_qubits <= 63, capacity <= 2^30.
 */
int naqs_ham_connected(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, int64_t row_begin, int64_t n_rows,
                       int64_t capacity, uint64_t *out_keys_dev, int64_t *count_dev, void *stream);

/*
 * Second-order Epstein-Nesbet terms of rows that need not be table rows.  The table S is keys_dev[M] (unique, physical, any
 * order, as for naqs_eloc) with real coefficients c_dev[M]; ext_keys_dev[n_ext] are the row keys (physical; usually the set
 * naqs_ham_connected returns, but a key of the table is allowed).  Per row a, both arrays optional (null: not returned):
 *   num_dev[a]  = sum over the non-diagonal XY groups g of H[a, a ^ xy_g] c[a ^ xy_g], over the partners the table holds —
 *                 the row walk of the E_loc kernel without its diagonal term and without a division; H[a, j] has the bits
 *                 naqs_eloc gives it;
 *   diag_dev[a] = H[a, a], the xy == 0 group (0 when the handle has none).
 * out4_dev[4] (mandatory), with den_a = e0 - diag_a:
 *   [0] sum over den_a < 0 of num_a^2 / den_a  (E_PT2 when e0 is the subspace energy and the rows its external set),
 *   [1] sum over den_a < 0 of num_a^2,
 *   [2] the number of rows with den_a >= 0 or NaN ("intruders"), as a double,
 *   [3] sum of num_a^2 over those rows.
 * Intruder rows never enter [0]: nothing is divided by a non-negative denominator.  The sums are taken in one fixed order (no
 * floating-point atomics): the same bits on repetition.  A row's num and diag depend on its key, the SET of table keys and c
 * only — not on the table's order, the other rows or the kernel form (NAQS_STAGE, NAQS_BLOCK, the Bloom filter).
 * n_ext = 0: out4 = 0, NAQS_OK.  M < 1, n_ext < 0, a null required pointer or a non-finite e0: NAQS_ERR_INVALID.
 * M > 2^24 - 1 (as naqs_eloc) or n_ext > 2^30: NAQS_ERR_UNSUPPORTED.
 * The call rebuilds the handle's sample-key table (like naqs_eloc).  It stands in for no reference code: the reference stops
 * at the variational subspace energy of solve_H (src/optimizer/energy.py:762-786).
 */
int naqs_ham_pt2(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, const double *c_dev, double e0,
                 int64_t n_ext, const uint64_t *ext_keys_dev,
                 double *num_dev, double *diag_dev, double *out4_dev, void *stream);

/*
 * Selected CI: which rows of a naqs_ham_pt2 call join the subspace.  Rows a = 0 .. n_ext-1 with distinct keys ext_keys_dev[a],
 * num_dev[a] and diag_dev[a] (what naqs_ham_pt2 writes); the rule, every operation one float64 rounding:
 *   den_a = diag_a - e0;
 *   a is an INTRUDER if !(den_a > 0) or num_a is NaN, and then eps_a = +inf; otherwise eps_a = (num_a * num_a) / den_a;
 *   a is ELIGIBLE if eps_a > 0 and eps_a >= eps_min  (a row with num = +-0 never is);
 *   k <= 0 or no eligible row: nothing is selected;  k >= the number of eligible rows: every eligible row is selected;
 *   otherwise tau = the k-th largest eligible eps, cut = tau * (1 - tie_rtol) (the factor formed on the host, one device
 *   multiplication), and every eligible row with eps >= cut is selected.
 * A near-degenerate group at the cut is never split, so the count may exceed k by the size of that group; tie_rtol = 0 keeps
 * bit-equal ties together.  The result is a function of the SET of (key, num, diag): out_keys_dev holds the selected keys in
 * ascending row order (ascending keys when the rows are naqs_ham_connected's, sorted), count_dev[0] their number, count_dev[1]
 * the number of intruders among them.  count_dev[0] > capacity: overflow, as naqs_ham_connected reports it — the counts are
 * written, out_keys_dev is unspecified.  n_ext = 0: counts 0, NAQS_OK.  eps_min or tie_rtol negative or NaN, a non-finite e0,
 * a null required pointer, n_ext < 0 or capacity < 0: NAQS_ERR_INVALID.  n_ext > 2^30: NAQS_ERR_UNSUPPORTED.
 * tau comes from an exact radix select on the bit patterns of eps (integer atomics only): the same bits on repetition and in
 * both kernel forms (NAQS_SELECT_FORM: 0 chosen by n_ext, 1 one workgroup and one launch, 2 tiles over many workgroups; read
 * at every call, reported by naqs_ham_last_kernel).  Nothing is read back.  Scratch belongs to the handle; when the tiled form
 * meets more rows than any call before it on the handle the scratch is released and allocated anew behind a device
 * synchronisation (as naqs_ham_pt2 grows its rows) — no other call synchronises.
 * tie_rtol is meant in [0, 1).  Beyond, the rule is applied as written and means little: at 1 the cut is 0 — every eligible row —
 * or, with tau = +inf, NaN — no row; above 1 the cut is negative — every eligible row.
 */
int naqs_ham_pt2_select(naqs_ham_t *h, int64_t n_ext, const uint64_t *ext_keys_dev, const double *num_dev,
                        const double *diag_dev, double e0, int64_t k, double eps_min, double tie_rtol,
                        int64_t capacity, uint64_t *out_keys_dev, int64_t *count_dev /* [2] */, void *stream);

/*
 * The lowest eigenpair of H restricted to the M table keys keys_dev (unique, physical, any order), by a diagonally
 * preconditioned Davidson iteration in real float64.  H on the table must be symmetric; d_i = H_ii; v0_dev[M] is the start.
 *
 *   v_0 = v0 / |v0| ;  w_0 = H v_0 ;  m = 1 ;  products = 1
 *   repeat
 *       G_kl = v_k . w_l  (k <= l, mirrored)            m x m
 *       (theta, s) = lowest eigenpair of G, |s| = 1
 *       x = sum_k s_k v_k ;  y = sum_k s_k w_k ;  r = y - theta x ;  rho = |r|
 *       rho < tol * max(1, |theta|)            -> status 0 (converged)
 *       m == M                                 -> status 2 (the basis spans the space; the pair is exact to rounding)
 *       products == max_products               -> status 1 (not converged; the pair is still returned)
 *       t_i = -r_i / max(d_i - theta, delta)
 *       m == m_max: restart                    V <- [x / |x|], W <- [y / |x|], m = 1
 *       twice:  t <- t - V (V^T t)
 *       |t| not finite, or <= 1e-14 * its norm before the two passes   -> status 3 (breakdown)
 *       v_m = t / |t| ;  w_m = H v_m ;  m += 1 ;  products += 1
 *   return theta, x / |x|, rho, products, status
 *
 * The correction is the positive-definite one: r / (theta - d), the textbook form, is a Newton step towards the eigenvalue
 * nearest theta and converges to excited states from a random start; with the denominator held at or above delta the step
 * always descends, and the iteration finds the lowest state of what v0 overlaps (a start that is an exact eigenvector is a
 * stationary point and is returned as such).
 * The product is the row walk of naqs_ham_pt2 over the table's own keys: H v = num + d * v, the key table built once per call.
 * The device forms w_m = (H t) / |t| where the rule writes H (t / |t|), the restart keeps x and y without the division by
 * |x| = 1 + O(2^-52), and G_00 after a restart is theta: each differs from the rule by roundings only.  The m x m problem is
 * solved by cyclic Jacobi in float64 in one workgroup.  Every sum over M runs in one fixed order (per-tile partial sums
 * combined in tile order, no floating-point atomics): the same inputs give the same bits on repetition, whatever the form of
 * the row walk's kernel.
 * vec_dev[M] receives x / |x|; info_host[4] (host memory) theta, rho, products, status.  The call synchronises the stream once
 * per product (eight words are read back) and once before the first.  Scratch — (2 m_max + 4) vectors of M doubles — belongs
 * to the handle and grows on demand behind a device synchronisation.  naqs_ham_last_kernel names the row walk's kernel and
 * the solver's.
 * NAQS_ERR_INVALID: M < 1, a null pointer, tol or delta not positive and finite, m_max outside 2 .. 32, max_products < 1, or a
 * zero or non-finite v0 (found on the device; no product is run and vec_dev is untouched).  NAQS_ERR_UNSUPPORTED: M > 2^24 - 1
 * (as naqs_ham_pt2).  It stands in for no reference code (the reference diagonalises the subspace with SciPy on the host).
 */
int naqs_ham_eig_lowest(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, const double *v0_dev, double tol,
                        int32_t max_products, int32_t m_max, double delta, double *vec_dev /* [M] */,
                        double info_host[4] /* theta, rho, products, status */, void *stream);

/*
 * The block product: nb (1 .. 8) coefficient vectors on ONE row walk over the M table keys keys_dev.
 *   C_dev   [nb][M]  vector c is the contiguous row c (real float64)
 *   num_dev [nb][M]  num[c][i] = sum_{j != i} H_ij C[c][j]
 *   diag_dev [M]     diag[i] = H_ii                      so that (H C[c])_i = num[c][i] + diag[i] * C[c][i]
 * Finding the partners of a key and forming H_ij does not depend on the vector, so the walk is made once: the vectors are first
 * laid out [M][4] (nb <= 4) or [M][8] in the handle's scratch — the padding columns zero —, and a hit reads one contiguous run
 * and does that many multiply-adds.  Column c of num_dev, and diag_dev, have the bits naqs_ham_pt2 gives with ext_keys_dev =
 * keys_dev and c_dev = row c, for every nb and every form of the walk (NAQS_STAGE, NAQS_BLOCK, the Bloom filter).
 * NAQS_ERR_INVALID: a null pointer, M < 1, nb outside 1 .. 8.  NAQS_ERR_UNSUPPORTED: M > 2^24 - 1 (as naqs_ham_pt2).  Nothing
 * is read back; the scratch grows on demand behind a device synchronisation.  naqs_ham_last_kernel names block_kernel's
 * instance.  It stands in for no reference code.
 */
int naqs_ham_block_product(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, int32_t nb, const double *C_dev,
                           double *num_dev, double *diag_dev, void *stream);

/*
 * The k = min(n_roots, M) lowest eigenpairs of H restricted to the M table keys, by a block Davidson iteration in real float64
 * with naqs_ham_eig_lowest's correction, tol and delta.  1 <= n_roots <= 8, 2 n_roots <= m_max <= 32; v0_dev [n_roots][M] holds
 * the starts, row j contiguous (the first k are used); d = diag H.
 *
 *   V = []                                      the start: the k rows of v0 in order
 *   for j < k:  t = v0_j ;  twice: t <- t - V^T (V t) ;  V += [t / |t|]
 *               |t| zero, not finite, or <= 1e-14 * its norm before the passes   -> NAQS_ERR_INVALID, no product is run
 *   W = H V ;  products = k
 *   repeat
 *       G = V W^T (upper triangle, mirrored) ;  its k lowest pairs (theta_j, s_j), theta ascending, equal ones by index
 *       x_j = s_j V ;  y_j = s_j W ;  r_j = y_j - theta_j x_j ;  rho_j = |r_j|
 *       open = [j : not rho_j < tol * max(1, |theta_j|)], ascending
 *       open empty -> status 0 ;  m == M -> status 2 ;  products >= max_products -> status 1
 *       m + len(open) > m_max: restart          V <- [x_j / |x_j|], W <- [y_j / |x_j|], j < k ;  m = k
 *       for j in open while m < M:
 *           t = -r_j / max(d - theta_j, delta)                     the positive form, for every root
 *           twice: t <- t - V^T (V t)                              V includes the vectors accepted earlier in this loop
 *           |t| not finite, or <= 1e-14 * its norm before the passes: skip this j
 *           V += [t / |t|] ;  W += [H t / |t|] ;  m += 1 ;  products += 1
 *       nothing accepted -> status 3
 *   return theta[k], x_j / |x_j|, rho[k], products, status
 *
 * With k = 1 this is naqs_ham_eig_lowest's rule.  Every loop iteration runs ONE block product (naqs_ham_block_product's walk,
 * the key table built once per call) over the corrections it accepted.  As in naqs_ham_eig_lowest the device forms (H t) / |t|,
 * keeps x_j and y_j at a restart without the division by |x_j| = 1 + O(2^-52) and sets G after a restart to diag(theta_j); a
 * correction accepted earlier in the loop is taken out of a later one as t_a (t_a . t) / |t_a|^2: each differs from the rule
 * by roundings only.  Every sum over M runs in one fixed order: the same bits on repetition and under every form of the walk.
 * vecs_dev [k][M] receives x_j / |x_j|; theta_host [k], rho_host [k] and info_host [2] = products, status are host memory.
 * The call synchronises the stream once per loop iteration (64 words are read back: the status and the accepted set) and once
 * for the start.  Scratch — (2 m_max + 4 k + 1) vectors of M doubles, and the block product's — belongs to the handle.
 * NAQS_ERR_INVALID: M < 1, a null pointer, tol or delta not positive and finite, n_roots outside 1 .. 8, m_max outside
 * 2 n_roots .. 32, max_products < 1, or a start that is rank-deficient, zero or not finite (found on the device; no product
 * is run and vecs_dev is untouched).  NAQS_ERR_UNSUPPORTED: M > 2^24 - 1.  It stands in for no reference code.
 */
int naqs_ham_eig_lowest_k(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, int32_t n_roots, const double *v0_dev, double tol,
                          int32_t max_products, int32_t m_max, double delta, double *vecs_dev /* [k][M] */,
                          double *theta_host /* [k] */, double *rho_host /* [k] */, int32_t info_host[2] /* products, status */,
                          void *stream);

/*
 * naqs_ham_pt2 for nb (1 .. 8) vectors of one table on ONE walk over the external rows: C_dev [nb][M] (row c contiguous, as
 * naqs_ham_block_product takes it) with the energies e_host [nb] (host memory); num_dev [nb][n_ext] (leading dimension n_ext)
 * and diag_dev [n_ext], both optional; out4_dev [nb][4] (mandatory).  Finding a row's partners and forming H[a, j] does not
 * depend on the vector, so the rows of all nb vectors come from one launch of naqs_ham_block_product's walk, its row list the
 * external keys, and their sums from one launch that reads diag once per row.
 * Row c of num_dev, diag_dev and out4_dev[c] have exactly the bits naqs_ham_pt2(h, M, keys_dev, C_dev[c], e_host[c], n_ext,
 * ext_keys_dev, ...) writes, for every nb and every form of the walk (NAQS_STAGE, NAQS_BLOCK, the Bloom filter); the key table
 * is built once per call.  Null num_dev / diag_dev: the handle's own scratch — naqs_ham_pt2's pair of arrays, grown as there.
 * n_ext = 0: out4 = 0, NAQS_OK.  nb outside 1 .. 8, M < 1, n_ext < 0, a null required pointer or a non-finite e_host[c]:
 * NAQS_ERR_INVALID.  M > 2^24 - 1 or n_ext > 2^30: NAQS_ERR_UNSUPPORTED.  naqs_ham_last_kernel names block_kernel's instance.
 * It stands in for no reference code.
 */
int naqs_ham_pt2_block(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, int32_t nb, const double *C_dev /* [nb][M] */,
                       const double *e_host /* [nb] */, int64_t n_ext, const uint64_t *ext_keys_dev,
                       double *num_dev /* [nb][n_ext], optional */, double *diag_dev /* [n_ext], optional */,
                       double *out4_dev /* [nb][4] */, void *stream);

/*
 * Selected CI for several roots: naqs_ham_pt2_select with the importances of nb (1 .. 8) roots averaged.  num_dev [nb][n_ext]
 * (leading dimension n_ext) and diag_dev [n_ext] are what naqs_ham_pt2_block writes; e_host [nb] and w_host [nb] (host memory)
 * the roots' energies and weights.  The rule, every operation one float64 rounding, no product and sum contracted:
 *   a root with w_j == 0 is skipped entirely (its row of num and its energy are never read); the others are LIVE, in ascending j;
 *   for each live j:  den_ja = diag_a - e_j ;  q_ja = (num_ja * num_ja) / den_ja;
 *   a is an INTRUDER if !(den_ja > 0) or num_ja is NaN for ANY live j, and then eps_a = +inf;
 *   otherwise eps_a = w_j0 * q_j0a for the first live root, then eps_a = eps_a + w_j * q_ja for each further live root in order.
 * Eligibility, tau, cut, the group at the cut that is never split, the row order of out_keys_dev, count_dev[2], overflow and
 * capacity are naqs_ham_pt2_select's, as are its two kernel forms (NAQS_SELECT_FORM), its scratch and its refusals;
 * NAQS_ERR_INVALID in addition for nb outside 1 .. 8, a weight that is negative or not finite, no live root, or a non-finite
 * e_j of a live root.
 * With nb = 1 and w = [1] the call selects exactly what naqs_ham_pt2_select selects, with the same counts (1 * q is exact);
 * with w = [1, 0, ...] what the single-root call on row 0 selects.  It stands in for no reference code.
 */
int naqs_ham_pt2_select_avg(naqs_ham_t *h, int64_t n_ext, const uint64_t *ext_keys_dev, int32_t nb, const double *num_dev,
                            const double *diag_dev, const double *e_host /* [nb] */, const double *w_host /* [nb] */, int64_t k,
                            double eps_min, double tie_rtol, int64_t capacity, uint64_t *out_keys_dev,
                            int64_t *count_dev /* [2] */, void *stream);

/* ---- inner ring: device versions of the three Cython entry points the reference imports ---- */

/* src.utils.hamiltonian_math.popcount_parity (hamiltonian_math.pyx:455-484):
 * out[i] = 1 - 2*(popcount(arr[i]) & 1), arr of signed ints with elem_bytes in {1,2,4,8} (the sign extension of a
 * narrow negative value adds an even number of bits, so unsigned arrays of the same width give the same parities). */
int naqs_popcount_parity(const void *arr_dev, int elem_bytes, int64_t n, int8_t *out_dev, void *stream);

/* src.utils.hamiltonian_math.get_Hij_cy (hamiltonian_math.pyx:198-288): dense matrix elements
 * hij_dev[i*Kxy + g] = H[i, key_i ^ xy_g] for M states, row-major, bit-identical to the reference
 * (same summation order). */
int naqs_get_hij(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, double *hij_dev, void *stream);

/* get_Hij_cy with the reference's own argument list (hamiltonian_math.pyx:198-288, body :85-100): the parity table
 * parity_dev int8 [M][Kyz] (= popcount_parity(key & unique_YZ)), and the K terms GROUPED BY OUTPUT COLUMN
 * (group_ptr_dev int32 [Kxy+1]; inside a column ascending original term index — a stable sort of unique2all_XY):
 * term_yz_dev int32 [K] = unique2all_YZ of the term, term_coeff_dev [K] float64 (coeff_bytes 8) or float32 (4).
 * hij_dev [M*Kxy] of the coupling type, hij[i*Kxy + g] = sum_{k in g} parity[i][yz(k)] * coeff[k], accumulated in
 * ascending k in the coupling type: bit-identical to the reference's loop.  naqs_amd/compat/hamiltonian_math.py. */
int naqs_hij_from_parity(int64_t M, int64_t Kxy, int64_t Kyz, int64_t K, const int8_t *parity_dev,
                         const int32_t *group_ptr_dev, const int32_t *term_yz_dev, const void *term_coeff_dev,
                         int coeff_bytes, void *hij_dev, void *stream);

/* src.utils.sparse_math.sparse_dense_mv (sparse_math.pyx:47-100): CSR (f64 data, int32 indices)
 * times complex128 vector; v_dev/out_dev are [.][2] = (Re, Im). */
int naqs_csr_mv(int64_t rows, const double *data_dev, const int32_t *indices_dev,
                const int32_t *indptr_dev, const double *v_dev, double *out_dev, void *stream);

/* ---- measurement ---- */

/* Record a hipEvent pair around every launch of the main E_loc kernel (up to max_records launches;
 * 0 disables and frees the events). */
int naqs_prof_enable(naqs_ham_t *h, int max_records);
/* Synchronises the recorded events: total milliseconds and number of launches since enable. */
int naqs_prof_read(naqs_ham_t *h, double *total_ms, int64_t *launches);
/* Name (with template arguments) of the local-energy kernel the handle's most recent call launched, e.g.
 * "eloc_kernel2<uint32_t, STAGE=2, NT=1024, BLOOM=0>"; empty before the first call.  Measurement aid (bench.py). */
int naqs_ham_last_kernel(const naqs_ham_t *h, char *buf, int buf_len);
/* How the handle's non-diagonal groups are evaluated by the default local-energy kernel: out[0] class D (double
 * excitations, one 16-entry sign table each), out[1] class S (single excitations, per-segment tables), out[2] class L
 * (the term loop), out[3] the bytes of the tables.  NAQS_ELOC_CLOSED=0 at creation puts every group in class L. */
int naqs_ham_closed_counts(const naqs_ham_t *h, int64_t out[4]);
/* The class and the table of ONE group (the terms that share the flip mask xy, in the order the handle keeps them: ascending
 * input position), as naqs_ham_create builds them; no device needed.  class_out: 0 L, 1 D, 2 S; ref_out: the reference
 * mask R; table_out (may be NULL): 16 doubles for class D, 4 * 64 * ceil(n_qubits / 6) for class S laid out
 * [segment][pattern][key slice], untouched for class L. */
int naqs_closed_group(int n_qubits, uint64_t xy, int64_t n_terms, const uint64_t *yz, const double *coeff,
                      int32_t *class_out, uint64_t *ref_out, double *table_out);
/* Record only every stride-th launch (default 1): an event pair costs a few microseconds of queue time,
 * so a sparse sample keeps the timed region representative. */
int naqs_prof_stride(naqs_ham_t *h, int stride);


/* ================================================================================================
 * Fused log-psi evaluation of the orbital NADE (inference; gradients stay with PyTorch autograd).
 * Replaces wavefunction.log_psi(states) (src/naqs/wavefunction.py:167-183) ->
 * _forward_predict (src/naqs/network/nade.py:738-770) for the published architecture family:
 * one amplitude MLP per orbital pair (one hidden layer; 2..4 of one width through naqs_net_create_amp_layers), and either
 * a single phase MLP on the last pair (aggregate_phase = False: -single_phase, the published runs) or one single-hidden-layer
 * phase block per pair whose outputs are summed (aggregate_phase = True: the reference's default; amplitude and phase blocks
 * both of 2..4 hidden layers through naqs_net_create_agg_layers), or no phase MLP and the
 * last amplitude block's output layer carrying the phase rows (naqs_net_create_combined: -single_phase -comb_amp_phase);
 * SoftmaxLogProbAmps amplitudes, with or without the phase spin symmetry.
 * ============================================================================================== */
typedef struct naqs_net naqs_net_t;

#define NAQS_NET_MAX_PAIRS 16
#define NAQS_NET_MAX_PHASE_LAYERS 8

typedef struct naqs_net_config {
    int32_t n_qubits;                 /* even, <= 2 * NAQS_NET_MAX_PAIRS */
    int32_t n_alpha, n_beta;          /* electron budget of the masks (nade.py:417-474); -1/-1: unrestricted */
    int32_t masking;                  /* NadeMasking: 0 NONE, 1 PARTIAL, 2 FULL (network/base.py:20-23) */
    int32_t use_amp_spin_sym;         /* 1: 5 amplitude outputs + symmetrisation (nade.py:576-594) */
    int32_t amp_hidden;               /* width of every hidden layer of every amplitude block */
    int32_t n_phase_hidden;           /* hidden layers of the phase block (>= 1) */
    int32_t phase_hidden[NAQS_NET_MAX_PHASE_LAYERS];   /* their widths */
    int32_t qubit2model[2 * NAQS_NET_MAX_PAIRS];       /* model position -> qubit (wavefunction.py:56-83, :369-383) */
    int32_t aggregate_phase;          /* 0: one phase MLP on the last pair (the published runs, -single_phase);
                                       * 1: one phase block per orbital pair, phases summed — the reference's default
                                       *    (experiments/run.py:31, nade.py:556-569): every block is
                                       *    Linear(max(1, 2n), phase_hidden[0]) + ReLU + Linear(phase_hidden[0], 4); n_phase_hidden must be 1
                                       *    (naqs_net_create_agg_layers: 1..4, the amplitude blocks' depth) */
    int32_t use_phase_spin_sym;       /* 1 (-phase_sym, nade.py:281, 507-533, 590-610; ABI 7): the phase block reads spin-ordered inputs
                                       *    (alpha and beta strings of the first P-1 pairs exchanged when idx(alpha) > idx(beta)), has
                                       *    3 outputs for |00>, |01> = |10>, |11>, and the phase gets + pi (N_01 mod 2) where
                                       *    idx(alpha) < idx(beta).  With aggregate_phase every per-pair block orders ITS prefix and
                                       *    the last block's phase carries the shift (nade.py:758-759). */
} naqs_net_config_t;

int naqs_net_create(const naqs_net_config_t *cfg, int device, naqs_net_t **out);
/* naqs_net_create for amplitude blocks of n_amp_hidden hidden layers, all cfg->amp_hidden wide (a multiple of 16, <= 128):
 * the reference's -n_layer (experiments/run.py; nade.py builds each block as n_layer Linear + ReLU groups and an output Linear).
 * n_amp_hidden == 1 is naqs_net_create.  NAQS_ERR_INVALID: n_amp_hidden outside 1..4; NAQS_ERR_UNSUPPORTED: aggregate_phase = 1
 * with n_amp_hidden > 1, or another width.  The flat layout stays the state_dict order, block by block
 * (amp_layers.<n>.layers.0.0.weight, .bias, amp_layers.<n>.layers.1.0.weight, ..., the output Linear), then the phase layers.
 * Every naqs_net_* / naqs_vmc_* entry point takes such a handle; the deep blocks run in launches of their own (the log-amplitude
 * launch in front of the phase kernel, one expand + scatter launch pair per sampler level, their own backward launch), so
 * naqs_vmc_step / naqs_vmc_run take the non-speculative order for them. */
int naqs_net_create_amp_layers(const naqs_net_config_t *cfg, int32_t n_amp_hidden, int device, naqs_net_t **out);
/* naqs_net_create for combined amplitude-phase blocks with a single phase (the reference's -single_phase -comb_amp_phase,
 * nade.py:294-303, 555-560): no phase MLP; every block is Linear(max(1, 2n), amp_hidden) + ReLU + Linear(amp_hidden, n_out), and
 * the last block's output layer has n_out_amp + n_out_phase rows — 5 + 3 with use_amp_spin_sym (spin-ordered inputs, the phase
 * row [0, 1, 1, 2][occ], + pi (N_01 mod 2)), 4 + 4 without; rows n_out_amp.. give the phase, earlier blocks contribute none.
 * NAQS_ERR_UNSUPPORTED: aggregate_phase = 1, or an amp_hidden that is not a multiple of 16 <= 128; NAQS_ERR_INVALID:
 * use_phase_spin_sym != use_amp_spin_sym (the reference forces them equal).  n_phase_hidden and phase_hidden are ignored.
 * The flat layout is the state_dict order, block by block; the last block is W1 [Ha][2(P-1)], b1 [Ha],
 * W2 [n_out_amp + n_out_phase][Ha], b2 [n_out_amp + n_out_phase].  naqs_net_param_count and naqs_net_amp_param_count both count
 * every parameter; naqs_net_set_amp_weights packs them all.  The sampler draws exactly what a naqs_net_create handle with the same
 * amplitude rows draws; naqs_net_amp_backward differentiates log|psi| only (zero gradient for the phase rows); naqs_vmc_step /
 * naqs_vmc_run take the non-speculative order; the naqs_vmc_shard_* calls return NAQS_ERR_UNSUPPORTED. */
int naqs_net_create_combined(const naqs_net_config_t *cfg, int device, naqs_net_t **out);
/* naqs_net_create for the aggregate phase (aggregate_phase = 1, the reference's default ansatz) with every block of n_hidden hidden
 * layers — the reference's -n_layer, which -n_layer_phase follows by default: amplitude blocks of cfg->amp_hidden units per layer,
 * per-pair phase blocks of cfg->phase_hidden[0] units per layer (each a multiple of 16, <= 128; the two may differ).
 * n_hidden == 1 is naqs_net_create.  NAQS_ERR_INVALID: cfg or out null, n_hidden outside 1..4 (or an odd n_qubits);
 * NAQS_ERR_UNSUPPORTED: aggregate_phase = 0 (naqs_net_create_amp_layers' family), cfg->n_phase_hidden != n_hidden,
 * phase_hidden[0 .. n_hidden - 1] not all equal, a width outside the set above, or P outside 2..16 — all of them before the device
 * is looked at.  The flat layout is the state_dict order: the amplitude blocks block by block (W1, b1, W2, b2, ..., Wo, bo as in
 * naqs_net_create_amp_layers), then the phase blocks the same way (Wo [4][Hp], or [3][Hp] with use_phase_spin_sym);
 * naqs_net_param_count counts both, naqs_net_amp_param_count the amplitude blocks.  The amplitude set is byte for byte a
 * naqs_net_create_amp_layers handle's, so the sampler, naqs_net_logamp and naqs_net_amp_backward run as for it;
 * naqs_net_set_amp_weights packs that set only.  naqs_net_last_kernel names the forward form ("agg_deep_kernel<CT, L=..>" when
 * both widths are equal, else "amp_deep_kernel<..> + amp_deep_raw_kernel<..>", then "+ agg_finish_kernel") and the last backward.
 * naqs_vmc_step / naqs_vmc_run take the non-speculative order; the naqs_vmc_shard_* calls return NAQS_ERR_UNSUPPORTED. */
int naqs_net_create_agg_layers(const naqs_net_config_t *cfg, int32_t n_hidden, int device, naqs_net_t **out);
int naqs_net_destroy(naqs_net_t *net);
/* Number of float parameters expected by naqs_net_set_weights: the reference's state_dict order,
 * flattened (amp_layers.0.layers.0.0.weight, .bias, amp_layers.0.layers.1.0.weight, .bias, ...,
 * phase_layers.0.layers.<l>.0.weight, .bias). */
int naqs_net_param_count(const naqs_net_t *net, int64_t *count);
/* Copy/re-pack the parameters (device pointer, float32, state_dict order) into the kernels' layout. */
int naqs_net_set_weights(naqs_net_t *net, const float *flat_dev, int64_t count, void *stream);
/* logpsi_dev: float [M][2] = (log|psi|, phase) for M keys. */
int naqs_net_logpsi(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, float *logpsi_dev, void *stream);
/*
 * The whole hot path of one VMC evaluation in one call: log psi of the M keys (naqs_net_logpsi) and their
 * local energies against the same table (naqs_eloc with NAQS_LOGPSI_F32 over all rows, + naqs_eloc_reduce
 * when w_dev/out4_dev are given).  The amplitude kernel inserts the keys into the E_loc hash table and the
 * phase kernel writes psi in float64, so the E_loc stage needs no preparation kernel of its own.
 * net and ham must live on the same device.  Results are identical to the two separate calls.
 */
int naqs_logpsi_eloc(naqs_net_t *net, naqs_ham_t *ham, int64_t M, const uint64_t *keys_dev,
                     const double *w_dev, float *logpsi_dev, double *eloc_dev, double *out4_dev, void *stream);

/*
 * Exact local energies of table rows [row_begin, row_begin + n_rows) in ONE call, device-resident: the training-time form of
 * the branch the reference leaves as `raise NotImplementedError()` (src/optimizer/energy.py:227-235, 250-258).  By definition
 * the sequence
 *   naqs_ham_connected(ham, M, keys, row_begin, n_rows, capacity, keys + M, &count)
 *   naqs_net_logpsi(net, count, keys + M, logpsi + M)
 *   naqs_eloc_reduced(ham, M + count, keys, logpsi, NAQS_LOGPSI_F32, row_begin, n_rows, w, eloc, out4)
 * with eloc_dev and out4_dev bit for bit what that sequence gives: the connected set is appended IN PLACE behind the table
 * (no copy, no concatenation, no sort: a row's hit set and summation order depend neither on what else the table holds nor
 * on its order, and the forward is row-independent), and the only thing the host learns is the count — published to a mapped
 * host word by a one-thread launch behind connected_kernel and read by a bounded poll (NAQS_SPIN_WAIT=0: the stream is
 * waited for instead), the way naqs_vmc_step learns M.  No workgroup waits for another.
 *
 * keys_dev   [M + capacity]: rows < M the table (input, unchanged); on return rows [M, M + count) hold the connected set
 *            of the range, in any order
 * logpsi_dev float [M + capacity][2]: rows < M input — log psi of the table from any forward of the handle's current
 *            parameters; rows [M, M + count) output, from the handle's inference forward (every family a handle can be)
 * eloc_dev   double [n_rows][2]
 * w_dev [n_rows], out4_dev [4]: both or neither; out4_dev <- the four weighted sums of the produced rows
 * info_host[0] = count (on overflow a lower bound, as in naqs_ham_connected), info_host[1] = 1 iff count > capacity.
 * On overflow the call returns NAQS_OK, nothing after the connected kernel is launched and eloc_dev, out4_dev and logpsi_dev
 * are untouched.  NAQS_ERR_UNSUPPORTED when M + count exceeds the 2^24 - 1 rows an E_loc table indexes; NAQS_ERR_INVALID
 * when net and ham do not live on the same device.
 */
int naqs_exact_eloc(naqs_net_t *net, naqs_ham_t *ham, int64_t M, uint64_t *keys_dev, float *logpsi_dev,
                    int64_t row_begin, int64_t n_rows, int64_t capacity, const double *w_dev,
                    double *eloc_dev, double *out4_dev, int64_t info_host[2], void *stream);

/* HIP-event timing of the phase-MLP kernel, like naqs_prof_enable / naqs_prof_read. */
int naqs_net_prof_enable(naqs_net_t *net, int max_records);
int naqs_net_prof_read(naqs_net_t *net, double *total_ms, int64_t *launches);
int naqs_net_prof_stride(naqs_net_t *net, int stride);
/* What the three calls above bracket: 0 (default) the log-psi kernel, 1 the sampler's launches of a training step (first
 * sampler launch .. the launch that writes the weights; naqs_vmc_step / naqs_vmc_run) — bench.py's `train_step.sampler_us`.
 * Selecting disarms the ring (enable it again afterwards). */
int naqs_net_prof_select(naqs_net_t *net, int which);
/* Kernel launches this library has issued in this process so far (all handles, all streams): bench.py's `launches per step`
 * is the difference over a timed region divided by its steps.  No counterpart in the reference. */
int64_t naqs_launch_count(void);
/* naqs_vmc_step / naqs_vmc_run launch the training forward behind the sampler's launches, BEFORE the host knows the number of
 * unique samples M (the kernel reads M on the device; the launch covers the last accepted draw's M plus an eighth in the kernel
 * form that M gets), and launch it again the ordinary way when the real M does not fit that launch or gets another form — the
 * same kernel on the same rows either way.  counts[0] = forwards launched ahead, counts[1] = of those, the ones that stood.
 * NAQS_SPEC_FORWARD=0: never ahead.  No counterpart in the reference (its loop is synchronous: energy.py:975-998). */
int naqs_net_spec_counts(const naqs_net_t *net, int64_t counts[2]);
/* Two (or more) handles driven from different threads / streams of ONE GPU — the farm's `experiments.run --farm --per-gpu 2`, no
 * counterpart in the reference, whose runs are one process each (experiments/bash/naqs/batch_train.sh:11-15).  on = 1: this
 * handle's sampler calls take turns with those of the device's other sharing handles: the sampler's look-back workgroups wait
 * for every workgroup before them, which is only certain to end while one such launch is in flight.  The turn
 * is held on the host (a spin lock per device, no event between the streams): naqs_vmc_step / naqs_vmc_run / 
 * naqs_vmc_sample_forward_eloc keep it from the sampler's first launch until they have read the draw's size, which they wait for
 * anyway; naqs_net_sample / naqs_net_sample_weighted wait for `stream` to drain before they return (in this mode only).
 * on = 0: off; on = -1: leave as is.  Default: the value of NAQS_SHARED_GPU (0) when the handle was created.
 * turns (may be NULL) <- sampler calls of this handle so far that had to wait for another handle's turn to end.
 * The samples do not depend on the switch. */
int naqs_net_share_device(naqs_net_t *net, int on, int64_t *turns);
/* Name of the log-psi kernel the most recent naqs_net_logpsi / naqs_logpsi_eloc / training forward launched, followed by
 * " + <kernel>" for the amplitude launch in front of it (or the aggregate-phase launches, or the combined blocks' phase head and
 * sums: " + comb_head_kernel + comb_finish_kernel").  Handles of
 * naqs_net_create_amp_layers append "; sampler: ..." or "; backward: ..." for the deep launches of the most recent sampler or
 * amplitude-backward call. */
int naqs_net_last_kernel(const naqs_net_t *net, char *buf, int buf_len);


/* ================================================================================================
 * Autoregressive tree sampler on the device.
 * Replaces wavefunction.sample(n) (src/naqs/wavefunction.py:488-521) -> _forward_sample
 * (src/naqs/network/nade.py:632-736) with multinomial_arr (:20-37): n_samples draws from |psi|^2 as the unique
 * bit-strings with their multiplicities.  Children that violate the electron budget are dropped after the draw
 * exactly like the reference (:695), so sum(counts) <= n_samples.  Outputs are in (prefix, outcome) order, which is
 * ascending key order for qubit_ordering = -1 (the reference's order).
 *   keys_dev [max_unique] uint64 (qubit order), counts_dev [max_unique] int64, probs_dev [max_unique] float32 or
 *   NULL (product of the float32 conditional probabilities, = the reference's `probs`),
 *   info_dev [2] int64: {number of unique samples M, overflow flag}.  overflow = 1 (and M = 0) when more than
 *   max_unique prefixes were alive at some level — the reference's MaxBatchSizeExceededError (:710-712).
 * Draws are a pure function of (weights, n_samples, seed): Philox4x32-10 keyed by the seed and indexed by the
 * prefix, exact binomials (inversion / BTRS).  Parity with the reference is statistical (numpy's generator is not
 * reproduced).  n_samples <= 2^44 (the float64 acceptance test of the binomial generator loses its margin beyond; the
 * reference caps n_samples at 1e12).
 * ============================================================================================== */
int naqs_net_sample(naqs_net_t *net, int64_t n_samples, uint64_t seed, int64_t max_unique, uint64_t *keys_dev,
                    int64_t *counts_dev, float *probs_dev, int64_t *info_dev, void *stream);

/* naqs_net_sample that also writes the samples' weights counts / sum(counts) (float64 [max_unique]; the `weights`
 * of PartialSamplingOptimizer.run, src/optimizer/energy.py:993) from the same final launch — the integer total is
 * exact, so the weights do not depend on a summation order. */
int naqs_net_sample_weighted(naqs_net_t *net, int64_t n_samples, uint64_t seed, int64_t max_unique, uint64_t *keys_dev,
                             int64_t *counts_dev, float *probs_dev, double *weights_dev, int64_t *info_dev, void *stream);

/* ================================================================================================
 * Training-time amplitude network: forward and backward of log|psi| in two launches each.
 * The reference back-propagates 2 Re sum_i w_i log psi_i (E_loc_i - <E>)^* through PyTorch autograd
 * (src/optimizer/energy.py:329-343); the amplitude half of that graph — ~10 orbital pairs x (2 Linear + mask +
 * log-softmax + gathers), src/naqs/network/nade.py:738-770 — is what these replace (the phase MLP is three plain
 * Linear layers and stays with the BLAS library).  Gradients are deterministic (fixed-order reductions).
 * ============================================================================================== */
/* Number of amplitude-block parameters = the leading part of the flat state_dict order of naqs_net_param_count. */
int naqs_net_amp_param_count(const naqs_net_t *net, int64_t *count);
/* Re-pack only the amplitude blocks (flat_dev: the whole flat parameter vector or just its amplitude part).
 * The packed phase layers become stale: naqs_net_logpsi / naqs_logpsi_eloc return NAQS_ERR_INVALID until the next
 * naqs_net_set_weights.  Enough for naqs_net_sample, naqs_net_logamp and naqs_net_amp_backward. */
int naqs_net_set_amp_weights(naqs_net_t *net, const float *flat_dev, int64_t count, void *stream);
/* logamp_dev [M] float32: log|psi(key_i)| (identical to column 0 of naqs_net_logpsi). */
int naqs_net_logamp(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, float *logamp_dev, void *stream);
/* grad_dev [amp_param_count] float32 (state_dict order) = d/d theta  sum_i g_dev[i] * log|psi(key_i)|. */
int naqs_net_amp_backward(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, const float *g_dev, float *grad_dev,
                          void *stream);

/* The whole network, forward and backward, for one batch of keys (no autograd graph):
 *   naqs_net_train_forward   = naqs_net_logpsi, and the phase MLP's inputs / hidden activations stay in the handle;
 *   naqs_net_train_backward  g_dev [M][2] float32 = d loss / d (log|psi_i|, phase_i)  ->  grad_dev [naqs_net_param_count]
 *                            float32 = d loss / d theta in state_dict order (amplitude blocks via naqs_net_amp_backward,
 *                            the phase Linear/ReLU stack as f32-MFMA GEMMs).  Must follow naqs_net_train_forward of the
 *                            SAME keys with no naqs_net_set_weights in between.  Deterministic. */
int naqs_net_train_forward(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, float *logpsi_dev, void *stream);
int naqs_net_train_backward(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, const float *g_dev, float *grad_dev,
                            void *stream);
/* naqs_vmc_loss_grad_ev + naqs_net_train_backward in ONE call (single-phase networks): the loss gradient g, its amplitude
 * column and the output layer's delta are written by one launch instead of three (vmc_grad, split, top-delta), then the backward
 * pass proper.  g_dev [M][2] and ev_dev [2] are outputs like naqs_vmc_loss_grad_ev's; grad_dev like naqs_net_train_backward's.
 * = loss.backward() of _SGD_step (src/optimizer/energy.py:328-343) given E_loc, the weights and the accumulators. */
int naqs_net_train_backward_vmc(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, const double *eloc_dev, const double *w_dev,
                                const double *sums_dev, float *g_dev, double *ev_dev, float *grad_dev, void *stream);
/* Natural-gradient training in sample space (minSR; no counterpart in the reference, whose two KFAC optimisers are unused).
 * With log psi_i = a_i + i phi_i, A = d a / d theta, B = d phi / d theta, weights w (sum 1), D = diag(sqrt w) and the seeds
 * g [M][2] of naqs_vmc_loss_grad:
 *   X_a = D (A - 1 w^T A), T_a = X_a X_a^T, y_a = g[:, 0] / (2 sqrt w); X_phi, T_phi, y_phi likewise from B and g[:, 1];
 *   d theta = X_a^T (T_a + lambda I)^-1 y_a + X_phi^T (T_phi + lambda I)^-1 y_phi, lambda = diag_shift * (mean diagonal of T).
 * naqs_net_sr_gram writes T_a + lambda I and T_phi + lambda I ([M][M] float64, symmetric) and y_a, y_phi ([M] float64);
 * naqs_net_sr_solve (below) or the caller's own library solves the two systems.  naqs_net_sr_direction forms the seeds s_i = sqrt(w_i) x_i - w_i sum_j sqrt(w_j) x_j per column and runs
 * naqs_net_train_backward with them: dir_dev [naqs_net_param_count] float32 = d theta.  Both must follow naqs_net_train_forward of
 * the SAME keys like naqs_net_train_backward.  The Gram matrices are built from per-layer float32 factors (no Jacobian) on the
 * float64 matrix cores (exact products, float64 sums in a fixed order): deterministic.  Memory: the caller's two M x M matrices (16 M^2 bytes) plus
 * O(M P Ha) floats of handle scratch; M > 32768 -> NAQS_ERR_UNSUPPORTED.  Single-phase and aggregate-phase handles with one hidden
 * layer per block; combined blocks (W1 shared between a and phi) and deeper blocks -> NAQS_ERR_UNSUPPORTED.  diag_shift <= 0, M < 1
 * or no training forward held -> NAQS_ERR_INVALID.  naqs_net_sr_gram_uncentred: G_a = A A^T and G_phi = B B^T as the kernels form
 * them, before centring — for tests and measurements. */
int naqs_net_sr_gram(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, const double *w_dev, const float *g_dev, double diag_shift,
                     double *Ta_dev, double *Tphi_dev, double *ya_dev, double *yphi_dev, void *stream);
int naqs_net_sr_gram_uncentred(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, double *Ga_dev, double *Gphi_dev, void *stream);
int naqs_net_sr_direction(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, const double *w_dev, const double *xa_dev,
                          const double *xphi_dev, float *dir_dev, void *stream);
/* The Jacobian-vector products of the same table: ua_dev [M] = A v and uphi_dev [M] = B v (float64, uncentred) for a vector
 * v_dev [naqs_net_param_count] float32 in state_dict order — the operand X phi_prev of a momentum step (SPRING: Goldshlager,
 * Abrahamsen, Lin 2024), centred by the caller as u - w^T u.  No Jacobian is formed: with layer l's per-sample factors
 * (delta_l,i, a_l,i) of naqs_net_sr_gram, (J v)_i = sum_l delta_l,i^T (V_l a_l,i + v_b,l), V_l and v_b,l the slices of v that are
 * the layer's weight and bias, read in place; float32 factors (the per-pair blocks' from a float64 evaluation, rounded once: the
 * training stage's d-out and d-pre are cancelling float32 sums) and v, exact products and float64 sums in a fixed order:
 * deterministic, and u_i depends on row i alone (the same bits at any M that holds the row).  The factors are recomputed by
 * every call.  Handles, preconditions and status codes as naqs_net_sr_gram_uncentred; a null pointer -> NAQS_ERR_INVALID. */
int naqs_net_sr_jvp(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, const float *v_dev, double *ua_dev, double *uphi_dev,
                    void *stream);
/* The solves between naqs_net_sr_gram and naqs_net_sr_direction: T x = y for the one or two symmetric positive definite [M][M]
 * row-major float64 matrices that naqs_net_sr_gram wrote, by a blocked Cholesky factorisation T = L L^T (64-wide block columns,
 * the trailing updates on the float64 matrix cores) and the forward and back substitutions, all in float64 — what
 * torch.linalg.cholesky_ex / torch.cholesky_solve do in the optimiser (naqs_amd/optimizer.py:833-837).  Asynchronous on
 * `stream`; both systems travel in the same 3 ceil(M / 64) launches.  Tphi_dev, yphi_dev and xphi_dev may be NULL together: one
 * system.  T is OVERWRITTEN: on return its lower triangle with the diagonal holds L, the strict upper triangle is unspecified.
 * x must not alias y or T; y is not written.  info_dev [2] int32, one word per system (both are written), LAPACK's potrf
 * convention: 0 = factorised, otherwise p + 1 for the first pivot p (0-based) with !(pivot > 0), so a NaN pivot fails too.  A
 * failed system's x is NaN throughout and its T is unspecified; the other system is unaffected bit for bit.  Deterministic: the
 * same bits on repetition, and for a system solved alone or beside another, in either slot.  `net` supplies the device and
 * 0.6 MB of scratch of its own (one solve at a time per handle): any family of handle, no training forward needed.
 * Null net, M < 1, a null required pointer or a partly null phi triple -> NAQS_ERR_INVALID; M > 32768 -> NAQS_ERR_UNSUPPORTED
 * (checked before any buffer is touched). */
int naqs_net_sr_solve(naqs_net_t *net, int64_t M, double *Ta_dev, double *Tphi_dev, const double *ya_dev, const double *yphi_dev,
                      double *xa_dev, double *xphi_dev, int32_t *info_dev, void *stream);
/* naqs_net_train_forward and the local energies of the same table in one call (= naqs_logpsi_eloc that also keeps the
 * activations for naqs_net_train_backward): the single-GPU training step's forward half, three launches. */
int naqs_net_train_forward_eloc(naqs_net_t *net, naqs_ham_t *ham, int64_t M, const uint64_t *keys_dev, const double *w_dev,
                                float *logpsi_dev, double *eloc_dev, double *out4_dev, void *stream);

/* One VMC step's first half in ONE call: naqs_net_sample_weighted, then — after the only host synchronisation of the step,
 * inside the library (the host has to learn M to size the launches) — naqs_net_train_forward_eloc of the sampled table.
 * Replaces wavefunction.sample + hilbert.state2idx + calculate_local_energy of PartialSamplingOptimizer.run
 * (src/optimizer/energy.py:975-998) as a sequence.  All `*_dev` outputs hold max_unique rows; rows >= M are unspecified.
 * info_host[0] = M, info_host[1] = overflow flag (then nothing was evaluated: MaxBatchSizeExceededError).  Between the
 * sampler's last kernel and the forward kernel the GPU waits for one stream synchronisation instead of for a return to
 * the caller's interpreter and a second library call. */
int naqs_vmc_sample_forward_eloc(naqs_net_t *net, naqs_ham_t *ham, int64_t n_samples, uint64_t seed, int64_t max_unique,
                                 uint64_t *keys_dev, int64_t *counts_dev, float *probs_dev, double *weights_dev,
                                 float *logpsi_dev, double *eloc_dev, double *out4_dev, int64_t *info_dev,
                                 int64_t info_host[2], void *stream);
/* ONE VMC training step in ONE call (single GPU, single-phase or aggregate-phase fused network):
 *   naqs_net_sample_weighted  ->  host learns (M, overflow)  ->  [accept M?]  ->  naqs_net_train_forward_eloc  ->
 *   naqs_net_train_backward_vmc  ->  naqs_adam_step on the flat parameter vector  ->  naqs_net_set_weights (re-pack).
 * = wavefunction.sample + calculate_local_energy + loss.backward() + optimizer.step() of PartialSamplingOptimizer.run /
 * _SGD_step (src/optimizer/energy.py:975-1008, :273-377).  The reference's adaptive sample count (energy.py:936-971) stays
 * with the caller: the step is abandoned after sampling — nothing evaluated, nothing updated — when the tree overflowed or
 * M is outside [m_lo, m_hi]; info_host[0] = M, [1] = overflow, [2] = 1 iff the step was taken.  adam_step < 1: stop after the
 * backward pass (the caller owns the optimiser).  The point of one call: between the sampler's last kernel and the re-pack
 * the GPU never waits for the caller's interpreter (measured: ~0.1 ms per step between the forward and the backward pass).
 * The one host/device rendezvous, M, is read from mapped host memory that the sampler writes as soon as the last level's size
 * is known (polled; NAQS_SPIN_WAIT=0: wait for the stream instead).  With adam_step >= 1 the reductions of the backward pass
 * apply Adam's update in the same launch (torch.optim.Adam's rule, as naqs_adam_step).
 * Re-pack: the kernels' packed copies of the updated parameters are made LATER, in stream order, from param_dev — inside the
 * next sampler call's first launch (whose own busy workgroup reads the four leading pairs' fragments: those are packed by the
 * update's launch itself), or at the start of whichever call of this handle first reads the amplitude blocks / the phase
 * layers (it starts the share it reads); a naqs_net_set_weights supersedes it.  param_dev must therefore stay allocated, and
 * unchanged unless naqs_net_set_weights follows, until one of those calls has been made (it is the optimiser's own parameter
 * vector in every caller here).  NAQS_PACK_OVERLAP=1: the amplitude blocks' share before the call returns, only the phase
 * layers' pending (ABI 6/7); 0: the whole re-pack before the call returns, as in ABI 5.  Same numbers in every form. */
int naqs_vmc_step(naqs_net_t *net, naqs_ham_t *ham, int64_t n_samples, uint64_t seed, int64_t max_unique, int64_t m_lo,
                  int64_t m_hi, uint64_t *keys_dev, int64_t *counts_dev, float *probs_dev, double *weights_dev,
                  float *logpsi_dev, double *eloc_dev, double *sums_dev, float *g_dev, double *ev_dev, float *grad_dev,
                  float *param_dev, float *exp_avg_dev, float *exp_avg_sq_dev, double lr, double beta1, double beta2,
                  double eps, double weight_decay, int64_t adam_step, int64_t info_host[3], void *stream);
/* The LOOP of PartialSamplingOptimizer.run (src/optimizer/energy.py:975-1008) around naqs_vmc_step, with get_samples'
 * adaptive sample count (energy.py:936-971) in C: n_steps training steps in ONE call, nothing returns to the caller's
 * interpreter in between.  Per step: draw with the current n_samples (seed of the k-th sampling call of the run =
 * splitmix64(seed_base + 0x9E3779B97F4A7C15 k), the rule of naqs_amd.wavefunction._next_sample_seed); while the library's
 * naqs_vmc_step abandons the draw — tree overflow (MaxBatchSizeExceededError, nade.py:710-712), or fewer than
 * n_unq_samples_min unique samples while the count may still grow — adapt n_samples x10 / /10 exactly as get_samples does and
 * draw again, recording an event per adaptation (the caller prints the reference's messages from them); then forward + E_loc,
 * backward, Adam, re-pack.  Everything a step leaves behind is what naqs_vmc_step leaves: the `*_dev` row buffers (max_unique =
 * n_unq_samples_max rows) hold the LAST step's table on return.  Per-step records: (<E>, Var) -> ev_log_dev[i][2] and the four
 * weighted sums -> sums_log_dev[i][4] (device, written in stream order), M / n_samples / host seconds since the call began ->
 * the three host arrays.  Sampled-state tracking (energy.py:300): with ring_elems > 0 step i's keys are written at
 * keys_dev + ring_off and ring_off advances by M; the run stops early (stop_reason 1) when the next step's max_unique keys would
 * not fit, so that the caller can fold the buffer.  stop_reason: 0 all n_steps taken, 1 tracking buffer full, 2 event buffer
 * full, 3 a draw was abandoned without a rule to adapt by (an error in the reference too).  steps_done steps were taken in any
 * case; Adam's step count, the sampling-call counter, n_samples and ring_off are updated in place.
 * Results are bit-identical to calling naqs_vmc_step step by step with the same seeds (tests/test_optimizer_gpu.py).
 * (continued below the type definitions) */
typedef struct naqs_vmc_event {
    int64_t step;            /* 0-based index (within this call) of the step whose draw was being adapted */
    int64_t n_unique;        /* unique samples of the abandoned draw (n_unq_samples_max + 1 for an overflow) */
    int32_t overflow;        /* 1: the tree overflowed (the reference prints "MaxBatchSizeExceededError") */
    int32_t action;          /* +1 n_samples x10, -1 n_samples /10, 0 unchanged (overflow right after an increase) */
    int64_t n_samples;       /* n_samples after the adaptation */
} naqs_vmc_event_t;
typedef struct naqs_vmc_run_args {
    /* sampling policy (in/out: n_samples, sample_calls) */
    int64_t n_samples, n_samples_max, n_unq_samples_min, n_unq_samples_max;
    uint64_t seed_base;
    int64_t sample_calls;
    /* Adam on the flat parameter vector (in/out: adam_step = updates applied so far) */
    float *param_dev, *exp_avg_dev, *exp_avg_sq_dev, *grad_dev;
    double lr, beta1, beta2, eps, weight_decay;
    int64_t adam_step;
    /* row buffers, n_unq_samples_max rows each (keys_dev: ring_elems elements when tracking) */
    uint64_t *keys_dev;
    int64_t ring_elems, ring_off;
    int64_t *counts_dev;
    float *probs_dev;
    double *weights_dev;
    float *logpsi_dev;
    double *eloc_dev;
    float *g_dev;
    /* per-step records, n_steps entries each */
    double *ev_log_dev, *sums_log_dev;
    int64_t *m_log_host, *ns_log_host;
    double *t_log_host;
    naqs_vmc_event_t *events;
    int64_t events_cap;
    /* out */
    int64_t n_events, steps_done, last_keys_off;
    int32_t stop_reason, pad;
} naqs_vmc_run_args_t;
int naqs_vmc_run(naqs_net_t *net, naqs_ham_t *ham, int64_t n_steps, naqs_vmc_run_args_t *args, void *stream);
/* naqs_device_check for ONE network handle: its own wait-failure word only (what a caller that shares the device with other
 * runs asks; ABI 8). */
int naqs_net_check(naqs_net_t *net);
/* Start a re-pack of the weights that a training step left pending (one that no launch has hosted yet) on `stream`; nothing
 * to do otherwise.  Every entry point that reads the packed weights does this itself.  No counterpart in the reference. */
int naqs_net_finish_pending(naqs_net_t *net, void *stream);
/* One Adam step on a flat float32 parameter vector (device pointers): torch.optim.Adam's rule without amsgrad —
 * the reference's optimiser, experiments/_base.py:228 (betas (0.9, 0.99), eps 1e-15).  `step` is the 1-based count
 * after this update (bias corrections 1 - beta^step are formed on the host in float64). */
int naqs_adam_step(int64_t n, float *param_dev, const float *grad_dev, float *exp_avg_dev, float *exp_avg_sq_dev,
                   double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, void *stream);
/* Inputs of the phase block from key bits: x_dev [M][2 (n_qubits/2 - 1)] float32 (+-1 occupations: alpha strings of
 * model pairs 0..P-2, then beta), occ_dev [M] int64 = realised outcome (alpha + 2 beta) of the last pair, which selects
 * the phase output (nade.py:563-569). */
int naqs_net_phase_inputs(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, float *x_dev, int64_t *occ_dev,
                          void *stream);
/* g_dev [M][2] float32 = d loss / d (log|psi_i|, phase_i) of the VMC loss 2 Re sum_i w_i log psi_i (E_loc_i - <E>)^*
 * (energy.py:328-329), <E> = (sums_dev[0], sums_dev[1]) as produced by naqs_eloc_reduce, evaluated in float32 like
 * the reference: (2 w Re(E_loc - <E>), -2 w Im(E_loc - <E>)).  eloc_dev [M][2] float64, w_dev [M] float64. */
int naqs_vmc_loss_grad(int64_t M, const double *eloc_dev, const double *w_dev, const double *sums_dev, float *g_dev,
                       void *stream);

/* naqs_vmc_loss_grad that also writes ev_dev[2] = { <E> = sums[0]/sums[3], Var = sums[2]/sums[3] - <E>^2 } (float64), the
 * two numbers _SGD_step returns (energy.py:372-375), from the same launch. */
int naqs_vmc_loss_grad_ev(int64_t M, const double *eloc_dev, const double *w_dev, const double *sums_dev, float *g_dev,
                          double *ev_dev, void *stream);

/* Multi-GPU step: the payload of the accumulator all-reduce, assembled in one launch — ext_dev[8] (float64) =
 * { sums_dev[0..4), M, M^2, c, c^2 } with c = (sum of the M keys) mod 2^20.  After a SUM over W ranks,
 * W * sum(x^2) == (sum x)^2 for x = M and x = c holds iff every rank contributed the same table (all values are exact
 * integers in float64): the per-step proof that the ranks row-sharded ONE table (the reference is single-process; the
 * counterpart is the `weights` / `sampled_idxs` bookkeeping of src/optimizer/energy.py:300, :993). */
int naqs_shard_proof(int64_t M, const uint64_t *keys_dev, const double *sums_dev, double *ext_dev, void *stream);

/* ---- the row-sharded training step (world > 1) as FOUR library calls with the three collectives in between (round 4) ----
 * One process per GPU; every rank draws the same table and owns the rows [b, e) = [min(M, rank S), min(M, (rank + 1) S)),
 * S = ceil(M / world) (src/optimizer/energy.py:273-377 split over ranks as SURVEY 8e describes).  The caller's sequence:
 *   naqs_vmc_shard_sample_forward          sampler -> host learns (M, overflow) -> [accept M?] -> training forward of MY rows,
 *                                          (log|psi|, phase) of them written to the front of `logpsi_shard_dev` (>= S rows)
 *   all-gather of the shards               -> table [world][S_pad][2] float32 (S_pad >= S: equal padded contributions)
 *   naqs_eloc_gathered                     prep (hash table, psi) straight from the gathered layout, E_loc of my rows against
 *                                          the whole table, weighted sums -> ext8[0..4), same-table proof -> ext8[4..8)
 *   all-reduce of ext8
 *   naqs_net_train_backward_vmc            loss gradient + backward of my rows (sums = the reduced ext8)
 *   all-reduce of the flat gradient
 *   naqs_vmc_shard_update                  Adam on the flat parameter vector + re-pack of the kernels' weight layouts
 * Same kernels and the same arithmetic as the call-by-call path of round 3 (energies and parameters agree bit for bit);
 * what goes is the interpreter time between the pieces — the GPU idled for it.  info_host[0] = M, [1] = overflow,
 * [2] = 1 iff the step was taken (M inside [m_lo, m_hi], no overflow; otherwise nothing was evaluated). */
int naqs_vmc_shard_sample_forward(naqs_net_t *net, int64_t n_samples, uint64_t seed, int64_t max_unique, int64_t m_lo, int64_t m_hi,
                                  int rank, int world, uint64_t *keys_dev, int64_t *counts_dev, float *probs_dev,
                                  double *weights_dev, float *logpsi_shard_dev, int64_t info_host[3], void *stream);
/* table_dev: [world][S_pad][2] float32 (log|psi|, phase), shard r = rows r S .. of the M-row table; w_dev, eloc_dev: MY rows
 * (n_rows entries, row_begin = my first row); ext8_dev: {sum w Re E, sum w Im E, sum w Re^2 E, sum w, M, M^2, c, c^2}
 * (naqs_eloc_reduced + naqs_shard_proof). */
int naqs_eloc_gathered(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, const float *table_dev, int64_t S, int64_t S_pad,
                       int64_t row_begin, int64_t n_rows, const double *w_dev, double *eloc_dev, double *ext8_dev, void *stream);
/* naqs_adam_step on the network's flat parameter vector followed by naqs_net_set_weights of the updated parameters. */
int naqs_vmc_shard_update(naqs_net_t *net, const float *grad_dev, float *param_dev, float *exp_avg_dev, float *exp_avg_sq_dev,
                          double lr, double beta1, double beta2, double eps, double weight_decay, int64_t adam_step,
                          void *stream);

/* Host evaluation of the sampler's generators, for known-answer and statistical tests (no device needed):
 * out[i] = Binomial(n, p) drawn from stream (seed, i);  Philox4x32-10 block function. */
int naqs_rng_binomial_host(int64_t n, double p, uint64_t seed, int64_t reps, int64_t *out);
int naqs_rng_philox_host(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);
/* The generator's own elementary functions on the host (the code the device runs, except for its refined reciprocal), for
 * accuracy tests: y[i] = f(x[i]) with fn 0: log (x > 0, normal), 1: log(1 - x) (0 < x <= 1/2), 2: exp (-745 < x <= 0),
 * 3: the uniform on (0, 1) made from the two 32-bit words packed in x[i]'s bit pattern (hi << 32 | lo). */
int naqs_rng_math_host(int fn, int64_t n, const double *x, double *y);
/* The sampler's GROUP draws on the device (the code a tree level runs: `group` = 4 lanes per draw as in the first split of a
 * prefix's count, 2 as in the second), for statistical tests: out_dev[i] = Binomial(n_dev[i % cases], p_dev[i % cases]) from
 * stream (seed, i), i < reps — neighbouring draws of a wave take different cases, so waves hold the inversion and the BTRS
 * regime side by side.  n <= 2^44.  No counterpart in the reference (numpy's generator, nade.py:20-37). */
int naqs_rng_binomial_device(int group, int cases, const int64_t *n_dev, const double *p_dev, uint64_t seed, int64_t reps,
                             int64_t *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NAQS_HIP_H */
