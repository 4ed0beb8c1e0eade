// naqs_sr_solve.hip — the two solves of the natural-gradient step (minSR) for gfx950 (MI355X):
//   naqs_net_sr_solve   T x = y for the one or two symmetric positive definite M x M float64 systems of naqs_net_sr_gram, by a
//                       blocked right-looking Cholesky factorisation T = L L^T (64-wide block columns) and the two substitutions
//
// Both systems travel in the same launches (blockIdx.z = system).  With nb = ceil(M / 64) block columns the chain on the one
// stream is   init | for k < nb: panel(k), update(k) | for k = nb - 1 .. 0: back(k)   = 3 nb launches, and the launch boundaries
// are the ONLY ordering between workgroups: no workgroup waits for another inside a launch.
//
//   sr_solve_init_kernel    info = 0, z = y (handle scratch; y is never written and x never aliases it), diagonal block 0 -> D
//   sr_chol_panel_kernel    step k, one workgroup per 64-row block of block column k and one for the right-hand side.  EVERY
//                           workgroup factorises the diagonal block itself: wave 0, lane = row, the row in 64 registers, column j
//                           broadcast with v_readlane — a 64-step chain without a barrier.  They read the block from the scratch
//                           copy D that the previous launch left, because workgroup 0 overwrites the block in T with L_kk in
//                           the same launch.  Then L_ik = A_ik L_kk^-T by substitution (four lanes per row, a quarter of the
//                           columns each), and z_k = L_kk^-1 (y_k - ...) as one more row: the forward substitution rides along.
//   sr_chol_update_kernel   A_ij -= L_ik L_jk^T for the 64 x 64 tiles j > k, i >= j on v_mfma_f64_16x16x4_f64 (four waves, 2 x 2
//                           MFMA tiles each, operands straight from memory: the depth is only 64), z_j -= L_jk z_k as one more
//                           row of tiles, and tile (k + 1, k + 1) also into D for the next panel launch.
//   sr_chol_back_kernel     step k of x = L^-T z: every workgroup solves x_k = L_kk^-T z_k itself (lane = column, 64-step chain),
//                           workgroup j < k takes z_j -= L_kj^T x_k, workgroup k writes x_k.
//
// info follows LAPACK's potrf: 0, or p + 1 for the first pivot p with !(pivot > 0) (a NaN pivot fails).  Only workgroup 0 of a
// panel launch writes it, having read it first; update and back launches read it and return at once for a failed system, whose x
// is filled with NaN.  Every loop's trip count is fixed by M, every sum has a fixed order, there are no atomics, and a system's
// arithmetic does not depend on its slot or on the other system: the same bits on repetition, alone or beside another.

#include <cmath>
#include <cstdint>
#include <limits>

#include "naqs_common.hpp"
#include "naqs_net.hpp"
#include "naqs_sr.hpp"

namespace {

using naqs::DeviceGuard;
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int NB = 64;                  // block edge
constexpr int LDL = NB + 1;             // row stride of the diagonal block in LDS (conflict-free for lane = row)
constexpr size_t SOLVE_SCRATCH_DOUBLES = 2 * (size_t)(NB * NB + naqs::SR_MAX_ROWS);   // per system: D [64][64], z [SR_MAX_ROWS]

struct SolveSys {
    double *T[2];                       // [M][M] row-major, overwritten by L
    double *D[2];                       // [64][64] the next diagonal block (handle scratch)
    double *z[2];                       // [M] the right-hand side on its way to L^-1 y (handle scratch)
    double *x[2];
    const double *y[2];
    int32_t *info;
};

// lane `src`'s value in every lane; src is the same in all lanes
__device__ __forceinline__ double bcast(const double v, const int src) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), src);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

__global__ __launch_bounds__(256) void sr_solve_init_kernel(const SolveSys S, const int64_t M) {
    const int sys = blockIdx.z;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < M) S.z[sys][i] = S.y[sys][i];
    if (blockIdx.x != 0) return;
    if (threadIdx.x == 0) {
        S.info[sys] = 0;
        if (gridDim.z == 1) S.info[1] = 0;
    }
    const int n = (int)(M < NB ? M : NB);
    for (int e = threadIdx.x; e < NB * NB; e += 256) {
        const int r = e >> 6, c = e & 63;
        if (r < n && c < n) S.D[sys][e] = S.T[sys][(int64_t)r * M + c];
    }
}

// The diagonal block in Ls ([64][LDL], rows and columns >= n are the identity's) -> its Cholesky factor in place (lower triangle
// and diagonal; the strict upper triangle is left as it falls).  Wave 0 only.  -> the first failed pivot of the block, or -1.
__device__ __forceinline__ int factor_diag_block(double *Ls, const int lane) {
    double row[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) row[c] = Ls[lane * LDL + c];
    int fail = -1;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const double d = bcast(row[j], j);
        if (!(d > 0.0) && fail < 0) fail = j;
        const double s = sqrt(d);
        row[j] = lane == j ? s : row[j] / s;
#pragma unroll
        for (int c = j + 1; c < NB; ++c) row[c] = fma(-row[j], bcast(row[j], c), row[c]);
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) Ls[lane * LDL + c] = row[c];
    return fail;
}

// Step k.  blockIdx.x = 0: the diagonal block (L_kk -> T, info); 1 .. nb - k - 1: block row k + blockIdx.x; nb - k: the
// right-hand side.  256 threads: thread (r = tid / 4, q = tid % 4) owns row r's columns 4 m + q.
__global__ __launch_bounds__(256) void sr_chol_panel_kernel(const SolveSys S, const int64_t M, const int k, const int nb) {
    __shared__ double Ls[NB * LDL];
    __shared__ double s_rdiag[NB];                      // 1 / L_cc: the substitution multiplies, as LAPACK's dtrsm does
    __shared__ int s_fail;
    const int sys = blockIdx.z, b = blockIdx.x, tid = threadIdx.x;
    if (b == 0 && S.info[sys] != 0) return;             // (the only writer of info reads it; the others factorise what they find)
    double *T = S.T[sys];
    const int64_t c0 = (int64_t)k * NB;
    const int n = (int)(M - c0 < NB ? M - c0 : NB);     // columns of this block column
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e >> 6, c = e & 63;
        Ls[r * LDL + c] = r < n && c < n ? S.D[sys][e] : (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    if (tid < 64) {
        const int fail = factor_diag_block(Ls, tid);
        s_rdiag[tid] = 1.0 / Ls[tid * LDL + tid];
        if (tid == 0) s_fail = fail;
    }
    __syncthreads();
    const int fail = s_fail;
    if (b == 0) {
        if (fail >= 0) {
            if (tid == 0) S.info[sys] = (int32_t)(c0 + fail + 1);
            return;
        }
        for (int e = tid; e < NB * NB; e += 256) {
            const int r = e >> 6, c = e & 63;
            if (c <= r && r < n) T[(c0 + r) * M + c0 + c] = Ls[r * LDL + c];
        }
        return;
    }
    if (fail >= 0) return;
    // rows x = a L_kk^-T: x_c = (a_c - sum_{j < c} x_j L_cj) (1 / L_cc), column by column; a_c' -= x_c L_c'c as soon as x_c is known
    const bool rhs = b == nb - k;
    const int r = tid >> 2, q = tid & 3, lane = tid & 63;
    double *base;
    bool live;
    if (rhs) { base = S.z[sys] + c0; live = r == 0; }
    else { const int64_t i0 = (int64_t)(k + b) * NB; base = T + (i0 + r) * M + c0; live = i0 + r < M; }
    double a[NB / 4];
#pragma unroll
    for (int m = 0; m < NB / 4; ++m) a[m] = live && 4 * m + q < n ? base[4 * m + q] : 0.0;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        const int m0 = c >> 2, q0 = c & 3;
        const double t = a[m0] * s_rdiag[c];
        const double xc = __shfl(t, (lane & ~3) | q0, 64);
        if (q == q0) a[m0] = xc;
        if (q > q0) a[m0] = fma(-xc, Ls[(4 * m0 + q) * LDL + c], a[m0]);
#pragma unroll
        for (int m = m0 + 1; m < NB / 4; ++m) a[m] = fma(-xc, Ls[(4 * m + q) * LDL + c], a[m]);
    }
    if (live) {
#pragma unroll
        for (int m = 0; m < NB / 4; ++m)
            if (4 * m + q < n) base[4 * m + q] = a[m];
    }
}

// Step k's trailing update.  grid (n, n + 1), n = nb - k - 1: tile (i, j) = (k + 1 + blockIdx.y, k + 1 + blockIdx.x) for
// blockIdx.y >= blockIdx.x, and blockIdx.y = n: the right-hand side's block j.  Operand maps as sr_tile_product (naqs_sr.hip):
// A: lane (m, q) holds -L_ik[row m][kk], B: L_jk[row m][kk]; D: col = lane & 15 (j), row = (lane >> 4) + 4 r (i).  Lane group q
// takes kk = 16 q + ks at step ks (the same for A and B, so the sum runs over all 64 in a fixed order) — 16 consecutive doubles
// of a row per lane.
__global__ __launch_bounds__(256) void sr_chol_update_kernel(const SolveSys S, const int64_t M, const int k) {
    const int sys = blockIdx.z, n = gridDim.x;
    if (S.info[sys] != 0) return;
    double *T = S.T[sys];
    const int64_t c0 = (int64_t)k * NB, j0 = (int64_t)(k + 1 + blockIdx.x) * NB;
    const int tid = threadIdx.x, lane = tid & 63;
    if ((int)blockIdx.y == n) {                           // z_j[c] -= sum_kk L_jk[c][kk] z_k[kk], kk ascending
        if (tid >= 64 || j0 + tid >= M) return;
        double *z = S.z[sys];
        const double *row = T + (j0 + tid) * M + c0;
        double v = z[j0 + tid];
        for (int kk = 0; kk < NB; ++kk) v = fma(-row[kk], z[c0 + kk], v);
        z[j0 + tid] = v;
        return;
    }
    if (blockIdx.y < blockIdx.x) return;
    const int64_t i0 = (int64_t)(k + 1 + blockIdx.y) * NB;
    const int wave = tid >> 6, wi = wave >> 1, wj = wave & 1, lm = lane & 15, lq = lane >> 4;
    double av[2][16], bv[2][16];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int64_t ri = i0 + wi * 32 + u * 16 + lm, rj = j0 + wj * 32 + u * 16 + lm;
        const double *pi = T + ri * M + c0 + 16 * lq, *pj = T + rj * M + c0 + 16 * lq;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            av[u][ks] = ri < M ? -pi[ks] : 0.0;
            bv[u][ks] = rj < M ? pj[ks] : 0.0;
        }
    }
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = i0 + wi * 32 + a * 16 + lq + 4 * r, j = j0 + wj * 32 + b * 16 + lm;
                acc[a][b][r] = i < M && j < M ? T[i * M + j] : 0.0;
            }
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0][ks], bv[0][ks], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0][ks], bv[1][ks], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1][ks], bv[0][ks], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1][ks], bv[1][ks], acc[1][1], 0, 0, 0);
    }
    const bool next_diag = blockIdx.x == 0 && blockIdx.y == 0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int li = wi * 32 + a * 16 + lq + 4 * r, lj = wj * 32 + b * 16 + lm;
                if (i0 + li < M && j0 + lj < M) {
                    T[(i0 + li) * M + j0 + lj] = acc[a][b][r];
                    if (next_diag) S.D[sys][li * NB + lj] = acc[a][b][r];
                }
            }
}

// Step k of the back substitution, one wave per workgroup, lane = column c of block k.  blockIdx.x = j <= k.
__global__ __launch_bounds__(64) void sr_chol_back_kernel(const SolveSys S, const int64_t M, const int k) {
    const int sys = blockIdx.z, j = blockIdx.x, c = threadIdx.x;
    const int64_t c0 = (int64_t)k * NB;
    const int n = (int)(M - c0 < NB ? M - c0 : NB);
    if (S.info[sys] != 0) {
        if (j == k && c < n) S.x[sys][c0 + c] = std::numeric_limits<double>::quiet_NaN();
        return;
    }
    const double *T = S.T[sys];
    double *z = S.z[sys];
    double col[NB];                                      // L_kk[r][c], r >= c (rows and columns >= n: the identity's)
#pragma unroll
    for (int r = 0; r < NB; ++r) col[r] = r < n && c < n ? T[(c0 + r) * M + c0 + c] : (r == c ? 1.0 : 0.0);
    const double rdiag = 1.0 / (c < n ? T[(c0 + c) * M + c0 + c] : 1.0);
    double acc = c < n ? z[c0 + c] : 0.0, x = 0.0;
#pragma unroll
    for (int r = NB - 1; r >= 0; --r) {                  // x_r = (z_r - sum_{r' > r} L[r'][r] x_r') (1 / L[r][r])
        const double t = acc * rdiag;
        const double xr = bcast(t, r);
        if (c == r) x = xr;
        if (c < r) acc = fma(-col[r], xr, acc);
    }
    if (j == k) {
        if (c < n) S.x[sys][c0 + c] = x;
        return;
    }
    const int64_t j0 = (int64_t)j * NB;                  // z_j[c] -= sum_r L_kj[r][c] x_k[r], r ascending
    double v = z[j0 + c];
#pragma unroll
    for (int r = 0; r < NB; ++r) {
        const double l = r < n ? T[(c0 + r) * M + j0 + c] : 0.0;
        v = fma(-l, bcast(x, r), v);
    }
    z[j0 + c] = v;
}

}  // namespace

NAQS_API int naqs_net_sr_solve(naqs_net_t *net, int64_t M, double *Ta_dev, double *Tphi_dev, const double *ya_dev,
                               const double *yphi_dev, double *xa_dev, double *xphi_dev, int32_t *info_dev, void *stream) {
    if (!net || M < 1 || !Ta_dev || !ya_dev || !xa_dev || !info_dev) return NAQS_ERR_INVALID;
    const int n_phi = (Tphi_dev ? 1 : 0) + (yphi_dev ? 1 : 0) + (xphi_dev ? 1 : 0);
    if (n_phi != 0 && n_phi != 3) return NAQS_ERR_INVALID;
    if (M > naqs::SR_MAX_ROWS) return NAQS_ERR_UNSUPPORTED;
    DeviceGuard guard;
    int st = guard.init(net->device);
    if (st != NAQS_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!net->d_sr_solve) {
        if (hipMalloc(&net->d_sr_solve, SOLVE_SCRATCH_DOUBLES * sizeof(double)) != hipSuccess) { net->d_sr_solve = nullptr; return NAQS_ERR_NOMEM; }
    }
    const unsigned n_sys = n_phi ? 2 : 1;
    SolveSys S{};
    double *scratch = static_cast<double *>(net->d_sr_solve);
    for (int k = 0; k < 2; ++k) {
        S.D[k] = scratch + (size_t)k * (NB * NB + naqs::SR_MAX_ROWS);
        S.z[k] = S.D[k] + NB * NB;
    }
    S.T[0] = Ta_dev; S.T[1] = Tphi_dev;
    S.y[0] = ya_dev; S.y[1] = yphi_dev;
    S.x[0] = xa_dev; S.x[1] = xphi_dev;
    S.info = info_dev;
    const int nb = (int)((M + NB - 1) / NB);
    NAQS_KLAUNCH(sr_solve_init_kernel, dim3((unsigned)((M + 255) / 256), 1, n_sys), dim3(256), 0, s, S, M);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < nb; ++k) {
        NAQS_KLAUNCH(sr_chol_panel_kernel, dim3((unsigned)(nb - k + 1), 1, n_sys), dim3(256), 0, s, S, M, k, nb);
        HIP_TRY(hipGetLastError());
        const unsigned n = (unsigned)(nb - k - 1);
        if (n == 0) continue;
        NAQS_KLAUNCH(sr_chol_update_kernel, dim3(n, n + 1, n_sys), dim3(256), 0, s, S, M, k);
        HIP_TRY(hipGetLastError());
    }
    for (int k = nb - 1; k >= 0; --k) {
        NAQS_KLAUNCH(sr_chol_back_kernel, dim3((unsigned)(k + 1), 1, n_sys), dim3(64), 0, s, S, M, k);
        HIP_TRY(hipGetLastError());
    }
    return NAQS_OK;
}
