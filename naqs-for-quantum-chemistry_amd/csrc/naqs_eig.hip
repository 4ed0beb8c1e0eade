// naqs_eig.hip — naqs_ham_eig_lowest: the lowest eigenpair of H restricted to a key table, by a diagonally preconditioned
// Davidson iteration (include/naqs_hip.h states the rule in full) — and, in the file's second half, naqs_ham_eig_lowest_k: the
// k lowest pairs by the block form of the same iteration, one block product per loop iteration.
//
// One product per iteration: H v = num + d * v from the row walk of naqs_ham_pt2 over the table's own keys (naqs_hip.hip:
// ham_eig_begin builds the key table once per solve, ham_eig_product launches pt2_kernel on it).  Around it five launches:
//   gram    tiles: v_m = t / |t|, w_m = (num + d t) / |t| (the normalisation folded in by linearity), the partial dots
//           v_k . w_m (k <= m) of every tile;
//   ritz    one workgroup: sums the partials in tile order, extends G, solves it (parallel-order cyclic Jacobi, float64, LDS),
//           writes theta and s;
//   expand  tiles: x = V s, y = W s, r = y - theta x, t = -r / max(d - theta, delta); the partials of |r|^2, |x|^2, |t|^2 and
//           V^T t; x is kept; at a restart x and y replace the basis in place;
//   orth    twice, tiles: every workgroup re-derives the coefficients V^T t from the previous launch's partials, in the same
//           order, takes them out of t and writes the next partials.  The first pass also settles the iteration: its workgroups
//           all form rho and the status from the partials, workgroup 0 writes them.
// House rules: no floating-point atomics, no workgroup waits for another, every sum over M in
// one fixed order (a thread's elements ascending, naqs_reduce.hpp's wave_sum, the waves in order, the tiles by tile_sums) — the
// same bits on repetition and whatever the form of the product's kernel.  One read-back of eight words per product.
//
// Layout: a vector is `ld` doubles, ld = M rounded up to even, so that every row of the basis is 16-byte aligned and a lane
// loads two elements at once; what lies at index M of an odd M is never trusted (load2 masks it) and always stored as zero.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "naqs_common.hpp"
#include "naqs_hash.hpp"
#include "naqs_reduce.hpp"

using namespace naqs;

namespace {

constexpr int EIG_BLOCK = 256;
constexpr int EIG_WAVES = EIG_BLOCK / WAVE;
constexpr int EIG_PAIRS = 4;                            // 16-byte loads a lane issues per vector
constexpr int EIG_TILE = EIG_BLOCK * EIG_PAIRS * 2;     // 2 048 elements a workgroup: 489 workgroups at M = 10^6 (256 CUs)
constexpr int EIG_MMAX = 32;
// a tile's partial sums: [0, 32) dots with the basis, then |r|^2, |x|^2, |t|^2
constexpr int P_R2 = EIG_MMAX, P_X2 = EIG_MMAX + 1, P_T2 = EIG_MMAX + 2, P_STRIDE = EIG_MMAX + 4;
// the status words (doubles).  STATUS: -1 go on, 0 / 1 / 2 as the rule, -2 a zero or non-finite start.  BRK: 1 = breakdown.
enum : int { W_THETA = 0, W_RHO = 1, W_STATUS = 2, W_BRK = 3, W_X2 = 4, W_TPRE2 = 5, W_COUNT = 8 };
constexpr int SMALL_DOUBLES = W_COUNT + EIG_MMAX + EIG_MMAX * EIG_MMAX;

struct EigArgs {
    int64_t M, ld;
    int32_t n_tiles;
    double *V, *W;                   // [m_max][ld] each
    double *d, *num, *t, *X;         // [ld] each
    const double *p_in;              // the previous launch's partials [n_tiles][P_STRIDE]
    double *p_out;                   // this launch's
    double *words, *s, *G;           // [W_COUNT], [32], [32][32]
};

__device__ __forceinline__ int64_t pair_index(const int j) {
    return (int64_t)blockIdx.x * EIG_TILE + ((int64_t)j * EIG_BLOCK + threadIdx.x) * 2;
}
// elements i, i + 1 (i even, i < M <= ld); the element at M is read as zero
__device__ __forceinline__ double2 load2(const double *p, const int64_t i, const int64_t M) {
    double2 v = *reinterpret_cast<const double2 *>(p + i);
    if (i + 1 >= M) v.y = 0.0;
    return v;
}
__device__ __forceinline__ void store2(double *p, const int64_t i, const double2 v) { *reinterpret_cast<double2 *>(p + i) = v; }

// Sums over the tiles of the partials [first, first + count) -> s_out[0 .. count).  Wave w takes the values w, w + 4, ...; lane l
// adds tiles l, l + 64, ... in ascending order, then wave_sum: one order whatever the grid.  Called by the whole workgroup.
template <int STRIDE = P_STRIDE>
__device__ __forceinline__ void tile_sums(const double *part, const int n_tiles, const int first, const int count, double *s_out) {
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    for (int v = wv; v < count; v += EIG_WAVES) {
        double a = 0.0;
        for (int tl = lane; tl < n_tiles; tl += WAVE) a += part[(size_t)tl * STRIDE + first + v];
        a = wave_sum(a);
        if (lane == 0) s_out[v] = a;
    }
    __syncthreads();
}

// One value of every thread -> the workgroup's sum, in s_red[slot][0 .. 4); added in wave order by whoever writes it out.
__device__ __forceinline__ void wave_part(const double a, double (*s_red)[EIG_WAVES], const int slot) {
    const double r = wave_sum(a);
    if ((threadIdx.x & (WAVE - 1)) == 0) s_red[slot][threadIdx.x / WAVE] = r;
}
__device__ __forceinline__ double wave_total(const double (*s_red)[EIG_WAVES], const int slot) {
    return (s_red[slot][0] + s_red[slot][1]) + (s_red[slot][2] + s_red[slot][3]);
}

// ---- the start: t = v0 (any alignment), the partials of |v0|^2 ----------------------------------------------------------------
__global__ __launch_bounds__(EIG_BLOCK) void eig_init_kernel(const EigArgs a, const double *__restrict__ v0) {
    __shared__ double s_red[1][EIG_WAVES];
    double n2 = 0.0;
#pragma unroll
    for (int j = 0; j < EIG_PAIRS; ++j) {
        const int64_t i = pair_index(j);
        if (i < a.M) {
            double2 v;
            v.x = v0[i];
            v.y = i + 1 < a.M ? v0[i + 1] : 0.0;
            store2(a.t, i, v);
            n2 += v.x * v.x;
            n2 += v.y * v.y;
        }
    }
    wave_part(n2, s_red, 0);
    __syncthreads();
    if (threadIdx.x == 0) a.p_out[(size_t)blockIdx.x * P_STRIDE + P_T2] = wave_total(s_red, 0);
}

// one workgroup: |v0|^2 -> the words of a fresh solve
__global__ __launch_bounds__(EIG_BLOCK) void eig_check_kernel(const EigArgs a) {
    __shared__ double s_n[1];
    tile_sums(a.p_in, a.n_tiles, P_T2, 1, s_n);
    if (threadIdx.x == 0) {
        const double n2 = s_n[0];
        const bool ok = n2 > 0.0 && n2 < __builtin_inf();
        a.words[W_THETA] = 0.0; a.words[W_RHO] = 0.0;
        a.words[W_STATUS] = ok ? -1.0 : -2.0;
        a.words[W_BRK] = 0.0;
        a.words[W_X2] = 1.0;
        a.words[W_TPRE2] = n2;
    }
}

// ---- gram: the product's result joins the basis as vector j ----------------------------------------------------------------
__global__ __launch_bounds__(EIG_BLOCK) void eig_gram_kernel(const EigArgs a, const int j) {
    __shared__ double s_n[1];
    __shared__ double s_red[EIG_MMAX + 1][EIG_WAVES];
    tile_sums(a.p_in, a.n_tiles, P_T2, 1, s_n);
    const double tn2 = s_n[0], tpre2 = a.words[W_TPRE2];
    // breakdown: |t| not finite, or not above 1e-14 of its norm before the two passes (every workgroup finds the same)
    if (!(tn2 < __builtin_inf()) || !(sqrt(tn2) > 1e-14 * sqrt(tpre2))) {
        if (blockIdx.x == 0 && threadIdx.x == 0) a.words[W_BRK] = 1.0;
        return;
    }
    const double scale = 1.0 / sqrt(tn2);
    double acc[EIG_MMAX], accd = 0.0;
#pragma unroll
    for (int k = 0; k < EIG_MMAX; ++k) acc[k] = 0.0;
    double *vj = a.V + (size_t)j * a.ld, *wj = a.W + (size_t)j * a.ld;
#pragma unroll
    for (int q = 0; q < EIG_PAIRS; ++q) {
        const int64_t i = pair_index(q);
        if (i < a.M) {
            const double2 tt = load2(a.t, i, a.M), nn = load2(a.num, i, a.M), dd = load2(a.d, i, a.M);
            double2 v, w;
            v.x = tt.x * scale; v.y = tt.y * scale;
            w.x = (nn.x + dd.x * tt.x) * scale; w.y = (nn.y + dd.y * tt.y) * scale;
            store2(vj, i, v);
            store2(wj, i, w);
            accd += v.x * w.x;
            accd += v.y * w.y;
#pragma unroll
            for (int k = 0; k < EIG_MMAX; ++k)
                if (k < j) {
                    const double2 vk = load2(a.V + (size_t)k * a.ld, i, a.M);
                    acc[k] += vk.x * w.x;
                    acc[k] += vk.y * w.y;
                }
        }
    }
#pragma unroll
    for (int k = 0; k < EIG_MMAX; ++k)
        if (k < j) wave_part(acc[k], s_red, k);
    wave_part(accd, s_red, EIG_MMAX);
    __syncthreads();
    double *out = a.p_out + (size_t)blockIdx.x * P_STRIDE;
    if ((int)threadIdx.x < j) out[threadIdx.x] = wave_total(s_red, threadIdx.x);
    if ((int)threadIdx.x == j) out[j] = wave_total(s_red, EIG_MMAX);
}

// ---- ritz: G extended by column j, its lowest eigenpair ---------------------------------------------------------------------
// Cyclic Jacobi in the round-robin order: n - 1 steps of n / 2 disjoint rotations a sweep (n even; an odd problem gets a row of
// zeros that no rotation touches).  Step r, pair q: (r, n - 1) for q = 0, else ((r + q) mod (n - 1), (r - q) mod (n - 1)) — every
// pair once a sweep.  A rotation's angle annihilates A[p][q] (Rutishauser's formulas); the columns of A and of the accumulated
// rotations turn first, then the rows of A, then the pair's owner writes the 2 x 2 block exactly.  A sweep without a rotation
// ends it: every off-diagonal element is then below the rounding of both its diagonal elements.
constexpr int JLD = EIG_MMAX + 1;
__global__ __launch_bounds__(EIG_BLOCK) void eig_ritz_kernel(const EigArgs a, const int j, const int restarted) {
    __shared__ double s_g[EIG_MMAX];
    __shared__ double A[EIG_MMAX][JLD], Q[EIG_MMAX][JLD];
    __shared__ double s_c[EIG_MMAX / 2], s_s[EIG_MMAX / 2];
    __shared__ int s_p[EIG_MMAX / 2], s_q[EIG_MMAX / 2];
    __shared__ int s_any, s_min;
    if (a.words[W_BRK] != 0.0) return;
    const int t = threadIdx.x;
    tile_sums(a.p_in, a.n_tiles, 0, j + 1, s_g);
    const int m = j + 1, n = (m + 1) & ~1;
    if (t <= j) {
        a.G[t * EIG_MMAX + j] = s_g[t];
        a.G[j * EIG_MMAX + t] = s_g[t];
    }
    if (restarted && t == 0) a.G[0] = a.words[W_THETA];        // after a restart v_0 = x, w_0 = y: v_0 . w_0 = theta
    __syncthreads();
    for (int e = t; e < n * n; e += EIG_BLOCK) {
        const int r = e / n, c = e % n;
        A[r][c] = (r < m && c < m) ? a.G[r * EIG_MMAX + c] : 0.0;
        Q[r][c] = r == c ? 1.0 : 0.0;
    }
    __syncthreads();
    const int half = n / 2;
    for (int sweep = 0; sweep < 60; ++sweep) {
        if (t == 0) s_any = 0;
        __syncthreads();
        for (int r = 0; r < n - 1; ++r) {
            double app = 0.0, aqq = 0.0, h = 0.0;
            int p = 0, q = 0;
            if (t < half) {
                p = t == 0 ? r : (r + t) % (n - 1);
                q = t == 0 ? n - 1 : (r - t + (n - 1)) % (n - 1);
                if (p > q) { const int x = p; p = q; q = x; }
                const double apq = A[p][q];
                app = A[p][p]; aqq = A[q][q];
                double c = 1.0, s = 0.0;
                const double g = 100.0 * fabs(apq);
                if (apq != 0.0 && !(fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq))) {
                    const double th = (aqq - app) / (2.0 * apq);
                    const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                    c = 1.0 / sqrt(tt * tt + 1.0);
                    s = tt * c;
                    h = tt * apq;
                    s_any = 1;
                }
                s_p[t] = p; s_q[t] = q; s_c[t] = c; s_s[t] = s;
            }
            __syncthreads();
            for (int e = t; e < n * half; e += EIG_BLOCK) {          // columns: A <- A J, Q <- Q J
                const int i = e / half, pr = e % half;
                const int pp = s_p[pr], qq = s_q[pr];
                const double c = s_c[pr], s = s_s[pr];
                const double x = A[i][pp], y = A[i][qq];
                A[i][pp] = c * x - s * y;
                A[i][qq] = s * x + c * y;
                const double u = Q[i][pp], v = Q[i][qq];
                Q[i][pp] = c * u - s * v;
                Q[i][qq] = s * u + c * v;
            }
            __syncthreads();
            for (int e = t; e < n * half; e += EIG_BLOCK) {          // rows: A <- J^T A
                const int i = e / half, pr = e % half;
                const int pp = s_p[pr], qq = s_q[pr];
                const double c = s_c[pr], s = s_s[pr];
                const double x = A[pp][i], y = A[qq][i];
                A[pp][i] = c * x - s * y;
                A[qq][i] = s * x + c * y;
            }
            __syncthreads();
            if (t < half) {
                A[p][p] = app - h;
                A[q][q] = aqq + h;
                A[p][q] = 0.0;
                A[q][p] = 0.0;
            }
            __syncthreads();
        }
        if (s_any == 0) break;                                        // (read by all after the step's last barrier)
        __syncthreads();
    }
    if (t == 0) {
        int best = 0;
        for (int k = 1; k < m; ++k)
            if (A[k][k] < A[best][best]) best = k;
        // (the padding row of an odd problem is index m: never a candidate)
        s_min = best;
    }
    __syncthreads();
    const int best = s_min;
    if (t == 0) {
        double n2 = 0.0, big = 0.0;
        for (int k = 0; k < m; ++k) {
            n2 += Q[k][best] * Q[k][best];
            if (fabs(Q[k][best]) > fabs(big)) big = Q[k][best];
        }
        const double f = (big < 0.0 ? -1.0 : 1.0) / sqrt(n2);
        for (int k = 0; k < m; ++k) a.s[k] = Q[k][best] * f;
        a.words[W_THETA] = A[best][best];
    }
}

// ---- expand: the Ritz vector, its residual, the correction ------------------------------------------------------------------
__global__ __launch_bounds__(EIG_BLOCK) void eig_expand_kernel(const EigArgs a, const int m, const int restart, const double delta) {
    __shared__ double s_s[EIG_MMAX];
    __shared__ double s_red[EIG_MMAX + 3][EIG_WAVES];
    if (a.words[W_BRK] != 0.0) return;
    if ((int)threadIdx.x < m) s_s[threadIdx.x] = a.s[threadIdx.x];
    __syncthreads();
    const double theta = a.words[W_THETA];
    double2 tq[EIG_PAIRS], xq[EIG_PAIRS];
    double r2 = 0.0, x2 = 0.0, t2 = 0.0;
#pragma unroll
    for (int q = 0; q < EIG_PAIRS; ++q) {
        const int64_t i = pair_index(q);
        tq[q] = make_double2(0.0, 0.0);
        xq[q] = make_double2(0.0, 0.0);
        if (i < a.M) {
            double2 x = make_double2(0.0, 0.0), y = make_double2(0.0, 0.0);
            for (int k = 0; k < m; ++k) {
                const double sk = s_s[k];
                const double2 vk = load2(a.V + (size_t)k * a.ld, i, a.M), wk = load2(a.W + (size_t)k * a.ld, i, a.M);
                x.x += sk * vk.x; x.y += sk * vk.y;
                y.x += sk * wk.x; y.y += sk * wk.y;
            }
            const double2 dd = load2(a.d, i, a.M);
            double2 r, tt;
            r.x = y.x - theta * x.x; r.y = y.y - theta * x.y;
            tt.x = -r.x / fmax(dd.x - theta, delta);
            tt.y = -r.y / fmax(dd.y - theta, delta);
            store2(a.t, i, tt);
            store2(a.X, i, x);
            if (restart) {
                store2(a.V, i, x);
                store2(a.W, i, y);
            }
            r2 += r.x * r.x; r2 += r.y * r.y;
            x2 += x.x * x.x; x2 += x.y * x.y;
            t2 += tt.x * tt.x; t2 += tt.y * tt.y;
            tq[q] = tt;
            xq[q] = x;
        }
    }
    // V^T t: against the basis as it stands for the passes — x alone after a restart
    double acc[EIG_MMAX];
#pragma unroll
    for (int k = 0; k < EIG_MMAX; ++k) acc[k] = 0.0;
    const int mv = restart ? 1 : m;
#pragma unroll
    for (int q = 0; q < EIG_PAIRS; ++q) {
        const int64_t i = pair_index(q);
        if (i < a.M) {
            if (restart) {
                acc[0] += xq[q].x * tq[q].x;
                acc[0] += xq[q].y * tq[q].y;
            } else {
#pragma unroll
                for (int k = 0; k < EIG_MMAX; ++k)
                    if (k < m) {
                        const double2 vk = load2(a.V + (size_t)k * a.ld, i, a.M);
                        acc[k] += vk.x * tq[q].x;
                        acc[k] += vk.y * tq[q].y;
                    }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < EIG_MMAX; ++k)
        if (k < mv) wave_part(acc[k], s_red, k);
    wave_part(r2, s_red, EIG_MMAX);
    wave_part(x2, s_red, EIG_MMAX + 1);
    wave_part(t2, s_red, EIG_MMAX + 2);
    __syncthreads();
    double *out = a.p_out + (size_t)blockIdx.x * P_STRIDE;
    if ((int)threadIdx.x < mv) out[threadIdx.x] = wave_total(s_red, threadIdx.x);
    if (threadIdx.x == P_R2) out[P_R2] = wave_total(s_red, EIG_MMAX);
    if (threadIdx.x == P_X2) out[P_X2] = wave_total(s_red, EIG_MMAX + 1);
    if (threadIdx.x == P_T2) out[P_T2] = wave_total(s_red, EIG_MMAX + 2);
}

// ---- orth: t <- t - V (V^T t), the coefficients re-derived by every workgroup ---------------------------------------------
struct EigDecide {
    int64_t m;                  // the basis the Ritz pair came from
    int32_t products, max_products;
    double tol;
};

template <bool FIRST>
__global__ __launch_bounds__(EIG_BLOCK) void eig_orth_kernel(const EigArgs a, const int mv, const EigDecide dc) {
    __shared__ double s_c[EIG_MMAX];
    __shared__ double s_n[3];
    __shared__ double s_red[EIG_MMAX + 1][EIG_WAVES];
    if (a.words[W_BRK] != 0.0) return;
    if (FIRST) {
        tile_sums(a.p_in, a.n_tiles, P_R2, 3, s_n);
        const double theta = a.words[W_THETA], rho = sqrt(s_n[0]);
        int status = -1;
        if (rho < dc.tol * fmax(1.0, fabs(theta))) status = 0;
        else if (dc.m == a.M) status = 2;
        else if (dc.products == dc.max_products) status = 1;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.words[W_RHO] = rho;
            a.words[W_X2] = s_n[1];
            a.words[W_TPRE2] = s_n[2];
            a.words[W_STATUS] = (double)status;
        }
        if (status >= 0) return;
    } else if (a.words[W_STATUS] >= 0.0) {
        return;
    }
    tile_sums(a.p_in, a.n_tiles, 0, mv, s_c);
    double2 tq[EIG_PAIRS];
    double t2 = 0.0;
#pragma unroll
    for (int q = 0; q < EIG_PAIRS; ++q) {
        const int64_t i = pair_index(q);
        tq[q] = make_double2(0.0, 0.0);
        if (i < a.M) {
            double2 tt = load2(a.t, i, a.M);
            for (int k = 0; k < mv; ++k) {
                const double ck = s_c[k];
                const double2 vk = load2(a.V + (size_t)k * a.ld, i, a.M);
                tt.x -= ck * vk.x;
                tt.y -= ck * vk.y;
            }
            store2(a.t, i, tt);
            t2 += tt.x * tt.x;
            t2 += tt.y * tt.y;
            tq[q] = tt;
        }
    }
    double *out = a.p_out + (size_t)blockIdx.x * P_STRIDE;
    if (FIRST) {
        double acc[EIG_MMAX];
#pragma unroll
        for (int k = 0; k < EIG_MMAX; ++k) acc[k] = 0.0;
#pragma unroll
        for (int q = 0; q < EIG_PAIRS; ++q) {
            const int64_t i = pair_index(q);
            if (i < a.M) {
#pragma unroll
                for (int k = 0; k < EIG_MMAX; ++k)
                    if (k < mv) {
                        const double2 vk = load2(a.V + (size_t)k * a.ld, i, a.M);
                        acc[k] += vk.x * tq[q].x;
                        acc[k] += vk.y * tq[q].y;
                    }
            }
        }
#pragma unroll
        for (int k = 0; k < EIG_MMAX; ++k)
            if (k < mv) wave_part(acc[k], s_red, k);
    }
    wave_part(t2, s_red, EIG_MMAX);
    __syncthreads();
    if (FIRST && (int)threadIdx.x < mv) out[threadIdx.x] = wave_total(s_red, threadIdx.x);
    if (threadIdx.x == EIG_MMAX) out[P_T2] = wave_total(s_red, EIG_MMAX);
}

// ---- the result: x / |x| into the caller's array (any alignment) ------------------------------------------------------------
__global__ __launch_bounds__(EIG_BLOCK) void eig_finish_kernel(const EigArgs a, double *__restrict__ vec) {
    const double f = 1.0 / sqrt(a.words[W_X2]);
#pragma unroll
    for (int q = 0; q < EIG_PAIRS; ++q) {
        const int64_t i = pair_index(q);
        if (i < a.M) {
            const double2 x = load2(a.X, i, a.M);
            vec[i] = x.x * f;
            if (i + 1 < a.M) vec[i + 1] = x.y * f;
        }
    }
}

// ==== naqs_ham_eig_lowest_k: the k lowest pairs, one block product per loop iteration ===========================================
// The launches of one iteration, in the style of the kernels above:
//   block product  num_c = (H - diag) t_c for the corrections accepted by the last chain, one row walk (naqs_hip.hip: block_kernel)
//   gramk    tiles: v_{m+c} = t_c / |t_c|, w_{m+c} = (num_c + d t_c) / |t_c|, the partial dots v_r . w_{m+c} (r <= m + c)
//   ritzk    one workgroup: G extended by up to k rows, cyclic Jacobi, the k lowest pairs ascending (ties by index)
//   expandk  tiles: x_j, y_j, r_j, t_j for every root; x_j, y_j and t_j are kept; the partials of |r_j|^2, |x_j|^2, |t_j|^2
//   settle   tiles: every workgroup forms rho_j, the open set, the status and the restart from the partials (workgroup 0 writes
//            them); at a restart each thread copies its elements of x_j, y_j over the basis; the dots V^T t_0
//   orthk    two per root, in root order: the pass takes the coefficients of the previous launch's partials out of t_j — the basis
//            rows and the corrections t_a (a < j) accepted before it, each as t_a (t_a . t_j) / |t_a|^2 —, and writes the dots the
//            next pass needs (of t_j again, or of t_{j+1}) and |t_j|^2.  A root that is closed, or has no room left (m = M), is
//            passed over: its launches only carry the next root's dots.  Whether t_a was accepted every workgroup re-derives from
//            |t_a|^2 before and after its passes, in the same way.
//   accept   one workgroup: the last root's acceptance, the accepted set, status 3 when it is empty
// and the iteration's one read-back (64 words): status, restart, the accepted set.  The start runs the same chain on the rows of
// v0 with an empty basis; a start row that is not accepted makes the call INVALID before any product.
constexpr int KR = 8;                                    // roots at most
constexpr int PK_STRIDE = KR * EIG_MMAX;                 // a tile's partials: gramk's [c][r]; the chain's below
constexpr int PK_T = EIG_MMAX, PK_N2 = EIG_MMAX + KR;    // chain: [0, 32) dots with the basis, [32, 40) with t_a, |t_cur|^2
constexpr int PE_R2 = 0, PE_X2 = KR, PE_T2 = 2 * KR;     // expandk: |r_j|^2, |x_j|^2, |t_j|^2
enum : int { KW_STATUS = 0, KW_RESTART = 1, KW_MV = 2, KW_NACC = 3, KW_THETA = 8, KW_RHO = 16, KW_X2 = 24, KW_TPRE2 = 32,
             KW_TN2 = 40, KW_OPEN = 48, KW_ACC = 56, KW_COUNT = 64 };
constexpr int SMALL_K_DOUBLES = KW_COUNT + KR * EIG_MMAX + EIG_MMAX * EIG_MMAX;

struct EigKArgs {
    int64_t M, ld;
    int32_t n_tiles, k;
    double *V, *W;                   // [m_max][ld] each
    double *d;                       // [ld]
    double *NUM, *T, *X, *Y;         // [k][ld] each
    const double *p_in;              // the previous launch's partials [n_tiles][PK_STRIDE]
    double *p_out;
    double *words, *S, *G;           // [KW_COUNT], [KR][32], [32][32]
};
struct EigKDecide {
    int64_t m;
    int32_t products, max_products, m_max, start;
    double tol;
};
struct EigKSlots { int32_t slot[KR]; };

// was the correction with |t|^2 = tn2 after its passes and tpre2 before them accepted (the rule's breakdown test, negated)
__device__ __forceinline__ bool kept(const double tn2, const double tpre2) {
    return tn2 < __builtin_inf() && sqrt(tn2) > 1e-14 * sqrt(tpre2);
}

// the dots of u (this thread's elements, uq) with the basis rows [0, mv) and the corrections t_a, a < nt -> the tile's partials
__device__ __forceinline__ void chain_dots(const EigKArgs &a, const double2 *uq, const int mv, const int nt, const double n2,
                                           double (*s_red)[EIG_WAVES]) {
    double acc[EIG_MMAX], acct[KR];
#pragma unroll
    for (int r = 0; r < EIG_MMAX; ++r) acc[r] = 0.0;
#pragma unroll
    for (int c = 0; c < KR; ++c) acct[c] = 0.0;
#pragma unroll
    for (int q = 0; q < EIG_PAIRS; ++q) {
        const int64_t i = pair_index(q);
        if (i < a.M) {
#pragma unroll
            for (int r = 0; r < EIG_MMAX; ++r)
                if (r < mv) {
                    const double2 vr = load2(a.V + (size_t)r * a.ld, i, a.M);
                    acc[r] += vr.x * uq[q].x;
                    acc[r] += vr.y * uq[q].y;
                }
#pragma unroll
            for (int c = 0; c < KR; ++c)
                if (c < nt) {
                    const double2 tc = load2(a.T + (size_t)c * a.ld, i, a.M);
                    acct[c] += tc.x * uq[q].x;
                    acct[c] += tc.y * uq[q].y;
                }
        }
    }
#pragma unroll
    for (int r = 0; r < EIG_MMAX; ++r)
        if (r < mv) wave_part(acc[r], s_red, r);
#pragma unroll
    for (int c = 0; c < KR; ++c)
        if (c < nt) wave_part(acct[c], s_red, PK_T + c);
    wave_part(n2, s_red, PK_N2);
    __syncthreads();
    double *out = a.p_out + (size_t)blockIdx.x * PK_STRIDE;
    const int t = threadIdx.x;
    if (t < mv || (t >= PK_T && t < PK_T + nt) || t == PK_N2) out[t] = wave_total(s_red, t);
}

// ---- the start: t_j = row j of v0 (any alignment), the partials of |v0_j|^2 ---------------------------------------------------
__global__ __launch_bounds__(EIG_BLOCK) void eigk_init_kernel(const EigKArgs a, const double *__restrict__ v0) {
    __shared__ double s_red[KR][EIG_WAVES];
    double n2[KR];
#pragma unroll
    for (int j = 0; j < KR; ++j) n2[j] = 0.0;
#pragma unroll
    for (int q = 0; q < EIG_PAIRS; ++q) {
        const int64_t i = pair_index(q);
        if (i < a.M) {
#pragma unroll
            for (int j = 0; j < KR; ++j)
                if (j < a.k) {
                    double2 v;
                    v.x = v0[(size_t)j * a.M + i];
                    v.y = i + 1 < a.M ? v0[(size_t)j * a.M + i + 1] : 0.0;
                    store2(a.T + (size_t)j * a.ld, i, v);
                    n2[j] += v.x * v.x;
                    n2[j] += v.y * v.y;
                }
        }
    }
#pragma unroll
    for (int j = 0; j < KR; ++j) wave_part(n2[j], s_red, j);
    __syncthreads();
    double *out = a.p_out + (size_t)blockIdx.x * PK_STRIDE;
    if (threadIdx.x < 2 * KR) out[threadIdx.x] = 0.0;
    if (threadIdx.x < KR) out[PE_T2 + threadIdx.x] = wave_total(s_red, threadIdx.x);
}

// ---- gramk: the block product's results join the basis as vectors m .. m + nnew - 1 ---------------------------------------------
__global__ __launch_bounds__(EIG_BLOCK) void eigk_gram_kernel(const EigKArgs a, const int m, const int nnew, const EigKSlots sl) {
    __shared__ double s_red[EIG_MMAX][EIG_WAVES];
    double *out = a.p_out + (size_t)blockIdx.x * PK_STRIDE;
    for (int c = 0; c < nnew; ++c) {
        const int j = m + c;
        const double scale = 1.0 / sqrt(a.words[KW_TN2 + sl.slot[c]]);
        const double *tc = a.T + (size_t)sl.slot[c] * a.ld, *nc = a.NUM + (size_t)c * a.ld;
        double *vj = a.V + (size_t)j * a.ld, *wj = a.W + (size_t)j * a.ld;
        double acc[EIG_MMAX];
#pragma unroll
        for (int r = 0; r < EIG_MMAX; ++r) acc[r] = 0.0;
#pragma unroll 1                                          // (unrolled: the loads of four pairs x 32 rows in flight, 360 registers)
        for (int q = 0; q < EIG_PAIRS; ++q) {
            const int64_t i = pair_index(q);
            if (i < a.M) {
                const double2 tt = load2(tc, i, a.M), nn = load2(nc, i, a.M), dd = load2(a.d, i, a.M);
                double2 v, w;
                v.x = tt.x * scale; v.y = tt.y * scale;
                w.x = (nn.x + dd.x * tt.x) * scale; w.y = (nn.y + dd.y * tt.y) * scale;
                store2(vj, i, v);
                store2(wj, i, w);
                // rows m .. j are this thread's own stores of this launch
#pragma unroll
                for (int r = 0; r < EIG_MMAX; ++r)
                    if (r <= j) {
                        const double2 vr = r == j ? v : load2(a.V + (size_t)r * a.ld, i, a.M);
                        acc[r] += vr.x * w.x;
                        acc[r] += vr.y * w.y;
                    }
            }
        }
#pragma unroll
        for (int r = 0; r < EIG_MMAX; ++r)
            if (r <= j) wave_part(acc[r], s_red, r);
        __syncthreads();
        if ((int)threadIdx.x <= j) out[c * EIG_MMAX + threadIdx.x] = wave_total(s_red, threadIdx.x);
        __syncthreads();
    }
}

// eig_ritz_kernel's sweeps as a function (that kernel keeps its own text: its device code is the parent's)
__device__ __forceinline__ void jacobi_sweeps(double (*A)[JLD], double (*Q)[JLD], double *s_c, double *s_s, int *s_p, int *s_q,
                                              int &s_any, const int n) {
    const int t = threadIdx.x;
    const int half = n / 2;
    for (int sweep = 0; sweep < 60; ++sweep) {
        if (t == 0) s_any = 0;
        __syncthreads();
        for (int r = 0; r < n - 1; ++r) {
            double app = 0.0, aqq = 0.0, h = 0.0;
            int p = 0, q = 0;
            if (t < half) {
                p = t == 0 ? r : (r + t) % (n - 1);
                q = t == 0 ? n - 1 : (r - t + (n - 1)) % (n - 1);
                if (p > q) { const int x = p; p = q; q = x; }
                const double apq = A[p][q];
                app = A[p][p]; aqq = A[q][q];
                double c = 1.0, s = 0.0;
                const double g = 100.0 * fabs(apq);
                if (apq != 0.0 && !(fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq))) {
                    const double th = (aqq - app) / (2.0 * apq);
                    const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                    c = 1.0 / sqrt(tt * tt + 1.0);
                    s = tt * c;
                    h = tt * apq;
                    s_any = 1;
                }
                s_p[t] = p; s_q[t] = q; s_c[t] = c; s_s[t] = s;
            }
            __syncthreads();
            for (int e = t; e < n * half; e += EIG_BLOCK) {          // columns: A <- A J, Q <- Q J
                const int i = e / half, pr = e % half;
                const int pp = s_p[pr], qq = s_q[pr];
                const double c = s_c[pr], s = s_s[pr];
                const double x = A[i][pp], y = A[i][qq];
                A[i][pp] = c * x - s * y;
                A[i][qq] = s * x + c * y;
                const double u = Q[i][pp], v = Q[i][qq];
                Q[i][pp] = c * u - s * v;
                Q[i][qq] = s * u + c * v;
            }
            __syncthreads();
            for (int e = t; e < n * half; e += EIG_BLOCK) {          // rows: A <- J^T A
                const int i = e / half, pr = e % half;
                const int pp = s_p[pr], qq = s_q[pr];
                const double c = s_c[pr], s = s_s[pr];
                const double x = A[pp][i], y = A[qq][i];
                A[pp][i] = c * x - s * y;
                A[qq][i] = s * x + c * y;
            }
            __syncthreads();
            if (t < half) {
                A[p][p] = app - h;
                A[q][q] = aqq + h;
                A[p][q] = 0.0;
                A[q][p] = 0.0;
            }
            __syncthreads();
        }
        if (s_any == 0) break;                                        // (read by all after the step's last barrier)
        __syncthreads();
    }
}

// ---- ritzk: G extended by nnew columns, its k lowest pairs ---------------------------------------------------------------------
__global__ __launch_bounds__(EIG_BLOCK) void eigk_ritz_kernel(const EigKArgs a, const int m, const int nnew, const int restarted) {
    __shared__ double s_g[PK_STRIDE];
    __shared__ double A[EIG_MMAX][JLD], Q[EIG_MMAX][JLD];
    __shared__ double s_c[EIG_MMAX / 2], s_s[EIG_MMAX / 2];
    __shared__ int s_p[EIG_MMAX / 2], s_q[EIG_MMAX / 2];
    __shared__ int s_any;
    const int t = threadIdx.x;
    tile_sums<PK_STRIDE>(a.p_in, a.n_tiles, 0, nnew * EIG_MMAX, s_g);
    // after a restart the basis is x_j, the products y_j (j < k = m): x_i . y_j = theta_j when i = j and 0 otherwise
    if (restarted && t < a.k * a.k) a.G[(t / a.k) * EIG_MMAX + t % a.k] = t / a.k == t % a.k ? a.words[KW_THETA + t / a.k] : 0.0;
    for (int e = t; e < nnew * EIG_MMAX; e += EIG_BLOCK) {
        const int j = m + e / EIG_MMAX, r = e % EIG_MMAX;
        if (r <= j) {
            a.G[r * EIG_MMAX + j] = s_g[e];
            a.G[j * EIG_MMAX + r] = s_g[e];
        }
    }
    __syncthreads();
    const int mm = m + nnew, n = (mm + 1) & ~1;
    for (int e = t; e < n * n; e += EIG_BLOCK) {
        const int r = e / n, c = e % n;
        A[r][c] = (r < mm && c < mm) ? a.G[r * EIG_MMAX + c] : 0.0;
        Q[r][c] = r == c ? 1.0 : 0.0;
    }
    __syncthreads();
    jacobi_sweeps(A, Q, s_c, s_s, s_p, s_q, s_any, n);
    if (t == 0) {
        // the k lowest diagonal elements in ascending order, equal ones by index (the padding row of an odd problem is index mm)
        uint32_t used = 0;
        for (int j = 0; j < a.k; ++j) {
            int best = -1;
            for (int c = 0; c < mm; ++c)
                if (!(used >> c & 1u) && (best < 0 || A[c][c] < A[best][best])) best = c;
            used |= 1u << best;
            double n2 = 0.0, big = 0.0;
            for (int r = 0; r < mm; ++r) {
                n2 += Q[r][best] * Q[r][best];
                if (fabs(Q[r][best]) > fabs(big)) big = Q[r][best];
            }
            const double f = (big < 0.0 ? -1.0 : 1.0) / sqrt(n2);
            for (int r = 0; r < mm; ++r) a.S[j * EIG_MMAX + r] = Q[r][best] * f;
            a.words[KW_THETA + j] = A[best][best];
        }
    }
}

// ---- expandk: every root's Ritz vector, residual and correction -----------------------------------------------------------------
__global__ __launch_bounds__(EIG_BLOCK) void eigk_expand_kernel(const EigKArgs a, const int m, const double delta) {
    __shared__ double s_S[KR][EIG_MMAX];
    __shared__ double s_th[KR];
    __shared__ double s_red[3 * KR][EIG_WAVES];
    for (int e = threadIdx.x; e < KR * EIG_MMAX; e += EIG_BLOCK)
        s_S[e / EIG_MMAX][e % EIG_MMAX] = (e / EIG_MMAX < a.k && e % EIG_MMAX < m) ? a.S[e] : 0.0;
    if (threadIdx.x < KR) s_th[threadIdx.x] = (int)threadIdx.x < a.k ? a.words[KW_THETA + threadIdx.x] : 0.0;
    __syncthreads();
    double r2[KR], x2[KR], t2[KR];
#pragma unroll
    for (int j = 0; j < KR; ++j) r2[j] = x2[j] = t2[j] = 0.0;
#pragma unroll 1
    for (int q = 0; q < EIG_PAIRS; ++q) {
        const int64_t i = pair_index(q);
        if (i < a.M) {
            double2 x[KR], y[KR];
#pragma unroll
            for (int j = 0; j < KR; ++j) x[j] = y[j] = make_double2(0.0, 0.0);
            for (int r = 0; r < m; ++r) {
                const double2 vr = load2(a.V + (size_t)r * a.ld, i, a.M), wr = load2(a.W + (size_t)r * a.ld, i, a.M);
#pragma unroll
                for (int j = 0; j < KR; ++j) {
                    const double sj = s_S[j][r];
                    x[j].x += sj * vr.x; x[j].y += sj * vr.y;
                    y[j].x += sj * wr.x; y[j].y += sj * wr.y;
                }
            }
            const double2 dd = load2(a.d, i, a.M);
#pragma unroll
            for (int j = 0; j < KR; ++j)
                if (j < a.k) {
                    const double theta = s_th[j];
                    double2 r, tt;
                    r.x = y[j].x - theta * x[j].x; r.y = y[j].y - theta * x[j].y;
                    tt.x = -r.x / fmax(dd.x - theta, delta);
                    tt.y = -r.y / fmax(dd.y - theta, delta);
                    store2(a.T + (size_t)j * a.ld, i, tt);
                    store2(a.X + (size_t)j * a.ld, i, x[j]);
                    store2(a.Y + (size_t)j * a.ld, i, y[j]);
                    r2[j] += r.x * r.x; r2[j] += r.y * r.y;
                    x2[j] += x[j].x * x[j].x; x2[j] += x[j].y * x[j].y;
                    t2[j] += tt.x * tt.x; t2[j] += tt.y * tt.y;
                }
        }
    }
#pragma unroll
    for (int j = 0; j < KR; ++j) {
        wave_part(r2[j], s_red, PE_R2 + j);
        wave_part(x2[j], s_red, PE_X2 + j);
        wave_part(t2[j], s_red, PE_T2 + j);
    }
    __syncthreads();
    double *out = a.p_out + (size_t)blockIdx.x * PK_STRIDE;
    if (threadIdx.x < 3 * KR) out[threadIdx.x] = wave_total(s_red, threadIdx.x);
}

// ---- settle: rho, the open set, the status, the restart; the first dots of the chain ----------------------------------------------
__global__ __launch_bounds__(EIG_BLOCK) void eigk_settle_kernel(const EigKArgs a, const EigKDecide dc) {
    __shared__ double s_e[3 * KR];
    __shared__ double s_red[PK_N2 + 1][EIG_WAVES];
    tile_sums<PK_STRIDE>(a.p_in, a.n_tiles, 0, 3 * KR, s_e);
    int status = -1, restart = 0, mv = 0, nopen = 0;
    uint32_t open = 0;
    if (dc.start) {
        open = (1u << a.k) - 1u;
    } else {
        for (int j = 0; j < a.k; ++j) {
            const double rho = sqrt(s_e[PE_R2 + j]);
            if (!(rho < dc.tol * fmax(1.0, fabs(a.words[KW_THETA + j])))) { open |= 1u << j; ++nopen; }
        }
        if (nopen == 0) status = 0;
        else if (dc.m == a.M) status = 2;
        else if (dc.products >= dc.max_products) status = 1;
        restart = status < 0 && dc.m + nopen > dc.m_max;
        mv = restart ? a.k : (int)dc.m;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < a.k) {
        const int j = threadIdx.x;
        a.words[KW_RHO + j] = sqrt(s_e[PE_R2 + j]);
        a.words[KW_X2 + j] = s_e[PE_X2 + j];
        a.words[KW_TPRE2 + j] = s_e[PE_T2 + j];
        a.words[KW_OPEN + j] = (double)(open >> j & 1u);
        a.words[KW_ACC + j] = 0.0;
        if (j == 0) {
            a.words[KW_STATUS] = (double)status;
            a.words[KW_RESTART] = (double)restart;
            a.words[KW_MV] = (double)mv;
            a.words[KW_NACC] = 0.0;
        }
    }
    if (status >= 0) return;
    double2 uq[EIG_PAIRS];
#pragma unroll
    for (int q = 0; q < EIG_PAIRS; ++q) {
        const int64_t i = pair_index(q);
        uq[q] = make_double2(0.0, 0.0);
        if (i < a.M) {
            if (restart)
                for (int j = 0; j < a.k; ++j) {
                    store2(a.V + (size_t)j * a.ld, i, load2(a.X + (size_t)j * a.ld, i, a.M));
                    store2(a.W + (size_t)j * a.ld, i, load2(a.Y + (size_t)j * a.ld, i, a.M));
                }
            uq[q] = load2(a.T, i, a.M);
        }
    }
    chain_dots(a, uq, mv, 0, 0.0, s_red);
}

// ---- orthk: one pass of root j ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EIG_BLOCK) void eigk_orth_kernel(const EigKArgs a, const int j, const int pass) {
    __shared__ double s_c[PK_N2 + 1];
    __shared__ double s_red[PK_N2 + 1][EIG_WAVES];
    if (a.words[KW_STATUS] >= 0.0) return;
    const int mv = (int)a.words[KW_MV];
    const bool settles = pass == 1 && j > 0;             // this launch is the first to see |t_{j-1}|^2 after its passes
    if (settles) tile_sums<PK_STRIDE>(a.p_in, a.n_tiles, PK_N2, 1, s_c + PK_N2);
    tile_sums<PK_STRIDE>(a.p_in, a.n_tiles, 0, mv, s_c);
    tile_sums<PK_STRIDE>(a.p_in, a.n_tiles, PK_T, j, s_c + PK_T);
    double inv[KR];
    int nacc = 0;
#pragma unroll
    for (int c = 0; c < KR; ++c) {
        inv[c] = 0.0;
        if (c < j) {
            const double tn2 = settles && c == j - 1 ? s_c[PK_N2] : a.words[KW_TN2 + c];
            const bool ok = a.words[KW_OPEN + c] != 0.0 && mv + nacc < a.M && kept(tn2, a.words[KW_TPRE2 + c]);
            if (settles && c == j - 1 && blockIdx.x == 0 && threadIdx.x == 0) a.words[KW_TN2 + c] = tn2;
            if (ok) { inv[c] = 1.0 / tn2; ++nacc; }
        }
    }
    const bool active = a.words[KW_OPEN + j] != 0.0 && mv + nacc < a.M;
    double *tj = a.T + (size_t)j * a.ld;
    const int nxt = pass == 1 ? j : j + 1;
    double2 uq[EIG_PAIRS];
    double n2 = 0.0;
#pragma unroll
    for (int q = 0; q < EIG_PAIRS; ++q) {
        const int64_t i = pair_index(q);
        uq[q] = make_double2(0.0, 0.0);
        if (i < a.M) {
            double2 tt = load2(tj, i, a.M);
            if (active) {
                for (int r = 0; r < mv; ++r) {
                    const double cr = s_c[r];
                    const double2 vr = load2(a.V + (size_t)r * a.ld, i, a.M);
                    tt.x -= cr * vr.x;
                    tt.y -= cr * vr.y;
                }
#pragma unroll
                for (int c = 0; c < KR; ++c)
                    if (c < j && inv[c] != 0.0) {
                        const double cc = s_c[PK_T + c] * inv[c];
                        const double2 tc = load2(a.T + (size_t)c * a.ld, i, a.M);
                        tt.x -= cc * tc.x;
                        tt.y -= cc * tc.y;
                    }
                store2(tj, i, tt);
                n2 += tt.x * tt.x;
                n2 += tt.y * tt.y;
            }
            uq[q] = nxt == j ? tt : (nxt < a.k ? load2(a.T + (size_t)nxt * a.ld, i, a.M) : make_double2(0.0, 0.0));
        }
    }
    chain_dots(a, uq, nxt < a.k ? mv : 0, nxt < a.k ? nxt : 0, n2, s_red);
}

// ---- accept: the last root's acceptance, the accepted set ---------------------------------------------------------------------
__global__ __launch_bounds__(EIG_BLOCK) void eigk_accept_kernel(const EigKArgs a) {
    __shared__ double s_n[1];
    if (a.words[KW_STATUS] >= 0.0) return;
    tile_sums<PK_STRIDE>(a.p_in, a.n_tiles, PK_N2, 1, s_n);
    if (threadIdx.x == 0) {
        const int mv = (int)a.words[KW_MV];
        int nacc = 0;
        for (int c = 0; c < a.k; ++c) {
            const double tn2 = c == a.k - 1 ? s_n[0] : a.words[KW_TN2 + c];
            const bool ok = a.words[KW_OPEN + c] != 0.0 && mv + nacc < a.M && kept(tn2, a.words[KW_TPRE2 + c]);
            a.words[KW_TN2 + c] = tn2;
            a.words[KW_ACC + c] = ok ? 1.0 : 0.0;
            nacc += ok;
        }
        a.words[KW_NACC] = (double)nacc;
        if (nacc == 0) a.words[KW_STATUS] = 3.0;
    }
}

// ---- the result: x_j / |x_j| into the caller's array (any alignment) -------------------------------------------------------------
__global__ __launch_bounds__(EIG_BLOCK) void eigk_finish_kernel(const EigKArgs a, double *__restrict__ vecs) {
    for (int j = 0; j < a.k; ++j) {
        const double f = 1.0 / sqrt(a.words[KW_X2 + j]);
#pragma unroll
        for (int q = 0; q < EIG_PAIRS; ++q) {
            const int64_t i = pair_index(q);
            if (i < a.M) {
                const double2 x = load2(a.X + (size_t)j * a.ld, i, a.M);
                vecs[(size_t)j * a.M + i] = x.x * f;
                if (i + 1 < a.M) vecs[(size_t)j * a.M + i + 1] = x.y * f;
            }
        }
    }
}

}  // namespace

NAQS_API int naqs_ham_eig_lowest(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, const double *v0_dev, double tol,
                                 int32_t max_products, int32_t m_max, double delta, double *vec_dev, double info_host[4], void *stream) {
    if (!h || M < 1 || !keys_dev || !v0_dev || !vec_dev || !info_host) return NAQS_ERR_INVALID;
    if (!(tol > 0) || !std::isfinite(tol) || !(delta > 0) || !std::isfinite(delta)) return NAQS_ERR_INVALID;
    if (m_max < 2 || m_max > EIG_MMAX || max_products < 1) return NAQS_ERR_INVALID;
    if (M > (1ll << 24) - 1) return NAQS_ERR_UNSUPPORTED;                 // naqs_ham_pt2's limit: 24-bit sample index
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DeviceGuard guard;
    int st = guard.init(ham_device(h));
    if (st != NAQS_OK) return st;

    EigArgs a;
    a.M = M;
    a.ld = (M + 1) & ~(int64_t)1;
    a.n_tiles = (int32_t)((M + EIG_TILE - 1) / EIG_TILE);
    const size_t part = (size_t)a.n_tiles * P_STRIDE;
    const int64_t need = (int64_t)((2 * (size_t)m_max + 4) * (size_t)a.ld + 2 * part + SMALL_DOUBLES);
    EigScratch *sc = ham_eig_scratch(h);
    if (need > sc->doubles) {
        st = regrow(sc->buf, sc->doubles, head_room(need, 1 << 16), (size_t)head_room(need, 1 << 16) * sizeof(double));
        if (st != NAQS_OK) return st;
    }
    double *at = sc->buf;                       // (hipMalloc aligns to 256 bytes; every piece below is an even number of doubles)
    a.V = at; at += (size_t)m_max * a.ld;
    a.W = at; at += (size_t)m_max * a.ld;
    a.d = at; at += a.ld;
    a.num = at; at += a.ld;
    a.t = at; at += a.ld;
    a.X = at; at += a.ld;
    double *p0 = at, *p1 = at + part;
    at += 2 * part;
    a.words = at; a.s = at + W_COUNT; a.G = a.s + EIG_MMAX;
    const dim3 grid((unsigned)a.n_tiles), block(EIG_BLOCK), one(1);
    auto args = [&](const double *in, double *out) { EigArgs b = a; b.p_in = in; b.p_out = out; return b; };

    ElocFeed feed;
    st = ham_eig_begin(h, M, keys_dev, s, &feed);
    if (st != NAQS_OK) return st;
    double words[W_COUNT];
    NAQS_KLAUNCH(eig_init_kernel, grid, block, 0, s, args(nullptr, p0), v0_dev);
    NAQS_KLAUNCH(eig_check_kernel, one, block, 0, s, args(p0, nullptr));
    HIP_TRY(hipMemcpyAsync(words, a.words, sizeof(words), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (words[W_STATUS] != -1.0) return NAQS_ERR_INVALID;                  // a zero or non-finite start: no product was run

    int m = 0, products = 0, restarted = 0, status = 3;
    for (;;) {
        st = ham_eig_product(h, M, keys_dev, feed, a.t, a.num, a.d, s);     // num = (H - diag) t, d = diag (the same bits every time)
        if (st != NAQS_OK) return st;
        ++products;
        NAQS_KLAUNCH(eig_gram_kernel, grid, block, 0, s, args(p0, p1), m);
        NAQS_KLAUNCH(eig_ritz_kernel, one, block, 0, s, args(p1, nullptr), m, restarted);
        ++m;
        const int restart = m == m_max ? 1 : 0, mv = restart ? 1 : m;
        NAQS_KLAUNCH(eig_expand_kernel, grid, block, 0, s, args(nullptr, p0), m, restart, delta);
        const EigDecide dc{(int64_t)m, products, max_products, tol};
        NAQS_KLAUNCH(eig_orth_kernel<true>, grid, block, 0, s, args(p0, p1), mv, dc);
        NAQS_KLAUNCH(eig_orth_kernel<false>, grid, block, 0, s, args(p1, p0), mv, dc);
        HIP_TRY(hipMemcpyAsync(words, a.words, sizeof(words), hipMemcpyDeviceToHost, s));   // the iteration's one read-back
        HIP_TRY(hipStreamSynchronize(s));
        if (words[W_BRK] != 0.0) {               // the correction vanished under the two passes: the product on it does not count
            --products;
            status = 3;
            break;
        }
        if (words[W_STATUS] >= 0.0) {
            status = (int)words[W_STATUS];
            break;
        }
        restarted = restart;
        if (restart) m = 1;
    }
    NAQS_KLAUNCH(eig_finish_kernel, grid, block, 0, s, args(nullptr, nullptr), vec_dev);
    HIP_TRY(hipGetLastError());
    info_host[0] = words[W_THETA];
    info_host[1] = words[W_RHO];
    info_host[2] = (double)products;
    info_host[3] = (double)status;
    char name[96];
    std::snprintf(name, sizeof(name), "%.50s + eig_gram, ritz, expand, orth x2 <T=%d>", ham_last_kernel_name(h), EIG_TILE);
    ham_set_last_kernel(h, name);
    return NAQS_OK;
}

NAQS_API int naqs_ham_eig_lowest_k(naqs_ham_t *h, int64_t M, const uint64_t *keys_dev, int32_t n_roots, const double *v0_dev, double tol,
                                   int32_t max_products, int32_t m_max, double delta, double *vecs_dev, double *theta_host,
                                   double *rho_host, int32_t info_host[2], void *stream) {
    if (!h || M < 1 || !keys_dev || !v0_dev || !vecs_dev || !theta_host || !rho_host || !info_host) return NAQS_ERR_INVALID;
    if (!(tol > 0) || !std::isfinite(tol) || !(delta > 0) || !std::isfinite(delta)) return NAQS_ERR_INVALID;
    if (n_roots < 1 || n_roots > KR || m_max < 2 * n_roots || m_max > EIG_MMAX || max_products < 1) return NAQS_ERR_INVALID;
    if (M > (1ll << 24) - 1) return NAQS_ERR_UNSUPPORTED;                 // naqs_ham_pt2's limit: 24-bit sample index
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DeviceGuard guard;
    int st = guard.init(ham_device(h));
    if (st != NAQS_OK) return st;

    EigKArgs a;
    a.M = M;
    a.ld = (M + 1) & ~(int64_t)1;
    a.n_tiles = (int32_t)((M + EIG_TILE - 1) / EIG_TILE);
    a.k = (int32_t)std::min<int64_t>(n_roots, M);
    const int k = a.k;
    const size_t part = (size_t)a.n_tiles * PK_STRIDE;
    const int64_t need = (int64_t)((2 * (size_t)m_max + 1 + 4 * (size_t)k) * (size_t)a.ld + 2 * part + SMALL_K_DOUBLES);
    EigScratch *sc = ham_eig_scratch(h);
    if (need > sc->doubles) {
        st = regrow(sc->buf, sc->doubles, head_room(need, 1 << 16), (size_t)head_room(need, 1 << 16) * sizeof(double));
        if (st != NAQS_OK) return st;
    }
    double *at = sc->buf;                       // (every piece is an even number of doubles: 16-byte aligned)
    a.V = at; at += (size_t)m_max * a.ld;
    a.W = at; at += (size_t)m_max * a.ld;
    a.d = at; at += a.ld;
    a.NUM = at; at += (size_t)k * a.ld;
    a.T = at; at += (size_t)k * a.ld;
    a.X = at; at += (size_t)k * a.ld;
    a.Y = at; at += (size_t)k * a.ld;
    double *p0 = at, *p1 = at + part;
    at += 2 * part;
    a.words = at; a.S = at + KW_COUNT; a.G = a.S + KR * EIG_MMAX;
    const dim3 grid((unsigned)a.n_tiles), block(EIG_BLOCK), one(1);
    auto args = [&](const double *in, double *out) { EigKArgs b = a; b.p_in = in; b.p_out = out; return b; };

    ElocFeed feed;
    st = ham_eig_begin(h, M, keys_dev, s, &feed);
    if (st != NAQS_OK) return st;
    double words[KW_COUNT];
    // settle, two passes a root, accept: the partials alternate between p0 and p1; the settle reads p0
    auto chain = [&](const EigKDecide &dc) -> int {
        double *in = p0, *out = p1;
        NAQS_KLAUNCH(eigk_settle_kernel, grid, block, 0, s, args(in, out), dc);
        std::swap(in, out);
        for (int j = 0; j < k; ++j)
            for (int pass = 1; pass <= 2; ++pass) {
                NAQS_KLAUNCH(eigk_orth_kernel, grid, block, 0, s, args(in, out), j, pass);
                std::swap(in, out);
            }
        NAQS_KLAUNCH(eigk_accept_kernel, one, block, 0, s, args(in, nullptr));
        HIP_TRY(hipMemcpyAsync(words, a.words, sizeof(words), hipMemcpyDeviceToHost, s));   // the iteration's one read-back
        HIP_TRY(hipStreamSynchronize(s));
        return NAQS_OK;
    };
    NAQS_KLAUNCH(eigk_init_kernel, grid, block, 0, s, args(nullptr, p0), v0_dev);
    st = chain(EigKDecide{0, 0, max_products, m_max, 1, tol});
    if (st != NAQS_OK) return st;
    if ((int)words[KW_NACC] != k) return NAQS_ERR_INVALID;   // a zero, non-finite or rank-deficient start: no product was run

    int m = 0, products = 0, restarted = 0, status = 3;
    for (;;) {
        EigKSlots sl;
        int nacc = 0;
        for (int j = 0; j < k; ++j)
            if (words[KW_ACC + j] != 0.0) sl.slot[nacc++] = j;
        for (int c = nacc; c < KR; ++c) sl.slot[c] = 0;
        st = ham_eig_block_product(h, M, keys_dev, feed, nacc, a.T, a.ld, sl.slot, a.NUM, a.ld, a.d, s);
        if (st != NAQS_OK) return st;
        products += nacc;
        NAQS_KLAUNCH(eigk_gram_kernel, grid, block, 0, s, args(nullptr, p0), m, nacc, sl);
        NAQS_KLAUNCH(eigk_ritz_kernel, one, block, 0, s, args(p0, nullptr), m, nacc, restarted);
        m += nacc;
        NAQS_KLAUNCH(eigk_expand_kernel, grid, block, 0, s, args(nullptr, p0), m, delta);
        st = chain(EigKDecide{(int64_t)m, products, max_products, m_max, 0, tol});
        if (st != NAQS_OK) return st;
        if (words[KW_STATUS] >= 0.0) {
            status = (int)words[KW_STATUS];
            break;
        }
        restarted = words[KW_RESTART] != 0.0 ? 1 : 0;
        if (restarted) m = k;
    }
    NAQS_KLAUNCH(eigk_finish_kernel, grid, block, 0, s, args(nullptr, nullptr), vecs_dev);
    HIP_TRY(hipGetLastError());
    for (int j = 0; j < k; ++j) {
        theta_host[j] = words[KW_THETA + j];
        rho_host[j] = words[KW_RHO + j];
    }
    info_host[0] = products;
    info_host[1] = status;
    char name[128];
    std::snprintf(name, sizeof(name), "%.60s + eigk_gram, ritz, expand, settle, orth, accept <T=%d>", ham_last_kernel_name(h), EIG_TILE);
    ham_set_last_kernel(h, name);
    return NAQS_OK;
}
