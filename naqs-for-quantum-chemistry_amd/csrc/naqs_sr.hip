// naqs_sr.hip — natural-gradient training in sample space (minSR) for gfx950 (MI355X):
//   naqs_net_sr_gram       keys, weights, loss seeds -> the two centred, shifted M x M Gram matrices T_a + lambda I,
//                          T_phi + lambda I and the right-hand sides y_a, y_phi (all float64)
//   naqs_net_sr_gram_uncentred  the two Gram matrices G_a, G_phi before centring (tests and measurements)
//   naqs_net_sr_direction  the solutions x_a, x_phi -> the natural-gradient direction, through naqs_net_train_backward
//   naqs_net_sr_jvp        a parameter-shaped vector v -> A v and B v (SPRING's momentum term), from the same factors
//
// With log psi_i = a_i + i phi_i, A = d a / d theta, B = d phi / d theta (M x N_p), D = diag(sqrt w):
//   X_a = D (A - 1 w^T A),  T_a = X_a X_a^T,  y_a = g[:, 0] / (2 sqrt w)   (likewise X_phi, T_phi, y_phi from B and g[:, 1])
//   d theta = X_a^T (T_a + lambda I)^-1 y_a + X_phi^T (T_phi + lambda I)^-1 y_phi
// The amplitude parameters move only a and the phase parameters only phi in the two supported families (single phase MLP,
// per-pair phase blocks), so the two blocks decouple.  No Jacobian is formed: every parameter sits in a Linear layer, a
// sample's gradient for it is delta_i (x) a_i, and the layer adds (Delta Delta^T) o (A A^T + 1) to the uncentred Gram matrix
// G = A A^T — two thin GEMMs over the sample axis and one elementwise product per layer.
//
//   sr_amp_factors_kernel  the backward pass's stage (1) (naqs_amp_backward.hpp: stage1_tile) on unit seeds, the tile written out
//                          instead of contracted: per pair and sample the block's inputs x (the bias as an explicit column of
//                          ones), hidden activations h, d-pre and d-out
//   sr_gram_kernel         one workgroup per 64 x 64 tile (I, J >= I): per factor pair both products of the float32 factors on
//                          v_mfma_f64_16x16x4_f64 (exact products, float64 sums), multiplied elementwise and accumulated in
//                          float64 in a fixed order.  G is then EXACTLY the Gram matrix of the float32 factors: T is positive
//                          semi-definite and T + lambda I factorises at any shift.  (On v_mfma_f32_16x16x4_f32 the two products
//                          come back rounded to float32 — 1.8e-7 of sqrt(G_ii G_jj) from float64 instead of 1.1e-7, as noise
//                          that is independent from element to element and that no Gram matrix has.)
//   sr_amp_factors64_kernel  for the Jacobian-vector product only: a block set's h, d-pre, d-out from a float64 evaluation, rounded once
//   sr_jvp_kernel          workgroups per 64-row tile: (J v)_i = sum_l delta_l,i^T (V_l a_l,i + v_b,l), V_l / v_b,l the slices of v
//                          that are layer l's weight / bias, read in place: per layer A_tile V_l^T on the same float64 MFMAs, the
//                          elementwise product with the deltas and a row sum in a fixed order; the (layer, 64 columns) items
//                          are dealt to up to 16 workgroups per tile, whose partial sums sr_jvp_sum_kernel adds in order
//   sr_rowsum_kernel       m = G w (fixed-order row sums), the diagonal, and the right-hand side
//   sr_center_kernel       T = D (G - m 1^T - 1 m^T + c) D + lambda I in place, c = w^T G w, lambda = diag_shift * tr T / M
//   sr_seeds_kernel        s_i = sqrt(w_i) x_i - w_i sum_j sqrt(w_j) x_j per column: X^T x = (backward pass with seeds s)
// Every sum has a fixed order and there are no float atomics: the results are deterministic.

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "naqs_common.hpp"
#include "naqs_net.hpp"
#include "naqs_amp_backward.hpp"
#include "naqs_sr.hpp"

namespace {

using naqs::MAXP;
using naqs::NetDims;
using naqs::SrJobs;
using naqs::WAVE;
using naqs::DeviceGuard;
using naqs::ampbw::GT;
using naqs::ampbw::LD;
using naqs::ampbw::MAX_DYN_LDS;
using namespace naqs::bwtile;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int TB = 64;       // Gram tile edge
constexpr int XLD = 64;      // leading dimension of the x and d-out factors; CH of their columns are written and read

// where pair n's factors of one block set go: [pair][cap rows][ld]
struct SrFactorOut { float *x, *dout, *h, *dh; int64_t cap; int ldh; };

// One orbital pair NB, all tiles of this workgroup: the backward pass's stage (1) on the seeds g (stride 2; the caller's are all
// 1), the tile it leaves in LDS written out as the pair's factors.  raw: the phase blocks of an aggregate-phase network.
template <int NB>
__device__ __forceinline__ void sr_factors_pair(const NetDims &d, const float *__restrict__ w, const int64_t M,
                                                const uint64_t *__restrict__ keys, const float *__restrict__ g, const SrFactorOut &F,
                                                float *smem, const int raw, const int wg, const int n_wgs) {
    constexpr int NIN = NB == 0 ? 1 : 2 * NB;
    static_assert(NIN + 1 <= CH, "the inputs and the bias fit one chunk of columns");
    const int Ha = d.Ha, NT = (Ha >> 4) * WAVE, tid = threadIdx.x;
    const naqs::ampbw::TileLds T = naqs::ampbw::tile_lds(Ha, naqs::amp_row_stride(NIN));
    const float *s_dpre = smem + T.dpre, *s_h = smem + T.h, *s_do = smem + T.dout;
    const uint32_t *s_x = reinterpret_cast<const uint32_t *>(smem + T.x);
    naqs::ampbw::stage_weights<NB>(d, w, smem);
    float *xo = F.x + (int64_t)NB * F.cap * XLD, *doo = F.dout + (int64_t)NB * F.cap * XLD;
    float *ho = F.h + (int64_t)NB * F.cap * F.ldh, *dho = F.dh + (int64_t)NB * F.cap * F.ldh;
    __syncthreads();

    for (int64_t t0 = (int64_t)wg * GT; t0 < M; t0 += (int64_t)n_wgs * GT) {
        float dout[5];
        naqs::ampbw::stage1_tile<NB>(d, smem, M, keys, g, 2, raw, t0, dout);
        // the tile's factors, row-major: consecutive threads take consecutive columns of a sample's row
        for (int e = tid; e < GT * Ha; e += NT) {
            const int r = e / Ha, j = e - r * Ha;
            if (t0 + r < M) {
                ho[(t0 + r) * F.ldh + j] = s_h[j * LD + r];
                dho[(t0 + r) * F.ldh + j] = s_dpre[j * LD + r];
            }
        }
        for (int e = tid; e < GT * CH; e += NT) {
            const int r = e / CH, c = e - r * CH;
            if (t0 + r < M) {
                const uint32_t xb = s_x[r];
                float xv = 0.0f;
                if (c < NIN) xv = NB == 0 ? 0.0f : (((xb >> c) & 1u) ? 1.0f : -1.0f);      // (pair 0: the constant-zero input)
                else if (c == NIN) xv = 1.0f;
                xo[(t0 + r) * XLD + c] = xv;
                doo[(t0 + r) * XLD + c] = c < 5 ? s_do[c * GT + r] : 0.0f;
            }
        }
        __syncthreads();
    }
}

// amp_backward_kernel's launch shape: workgroup = pair blockIdx.y x a strided set of 64-sample tiles, Ha / 16 waves
__global__ __launch_bounds__(512) void sr_amp_factors_kernel(const NetDims d, const float *__restrict__ w, const int64_t M,
                                                             const uint64_t *__restrict__ keys, const float *__restrict__ g,
                                                             const SrFactorOut F, const int raw) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    naqs::ampbw::for_pair((int)blockIdx.y, [&](auto nb) {
        sr_factors_pair<decltype(nb)::value>(d, w, M, keys, g, F, smem, raw, (int)blockIdx.x, (int)gridDim.x);
    });
}

// amp_block_delta for unit seeds in float64: d la[occ] / d o[c] from the block's raw outputs (raw: [c == phase_out_row(occ)])
__device__ __forceinline__ void sr_block_delta64(const NetDims &d, const int NB, const bool raw, const double (&o)[5], const uint32_t abits,
                                                 const uint32_t bbits, const int occ, double (&dout)[5]) {
    if (raw) {
#pragma unroll
        for (int c = 0; c < 5; ++c) dout[c] = c == naqs::phase_out_row(d, occ) ? 1.0 : 0.0;
        return;
    }
    const int x_order = abits > bbits ? 0 : (abits == bbits ? 1 : 2);
    double a4[4], da4[4];
    if (d.sym) {                                           // amp_symmetrise
        const double s1 = x_order == 0 ? o[3] : (x_order == 1 ? o[1] : o[4]);
        const double s2 = x_order == 0 ? o[4] : (x_order == 1 ? o[1] : o[3]);
        a4[0] = o[0]; a4[1] = (o[1] + s1) * 0.5; a4[2] = (o[1] + s2) * 0.5; a4[3] = o[2];
    } else {
        a4[0] = o[0]; a4[1] = o[1]; a4[2] = o[2]; a4[3] = o[3];
    }
    bool ok[4];
    if (!(d.masking == 0 || (d.masking == 1 && NB == d.P - 1))) naqs::amp_budget_mask(d, NB, abits, bbits, ok);
    else ok[0] = ok[1] = ok[2] = ok[3] = true;
    double m = -INFINITY, s = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) { a4[c] *= 2.0; if (ok[c]) m = fmax(m, a4[c]); }
#pragma unroll
    for (int c = 0; c < 4; ++c) if (ok[c]) s += exp(a4[c] - m);
    const bool live = occ == 0 ? ok[0] : (occ == 1 ? ok[1] : (occ == 2 ? ok[2] : ok[3]));
#pragma unroll
    for (int c = 0; c < 4; ++c) da4[c] = live && ok[c] ? (c == occ ? 1.0 : 0.0) - exp(a4[c] - m) / s : 0.0;
    dout[0] = dout[1] = dout[2] = dout[3] = dout[4] = 0.0;
    if (d.sym) {                                           // transpose of amp_symmetrise
        dout[0] = da4[0];
        dout[2] = da4[3];
        dout[1] = 0.5 * (da4[1] + da4[2]);
        if (x_order == 1) dout[1] += 0.5 * (da4[1] + da4[2]);
        else if (x_order == 0) { dout[3] = 0.5 * da4[1]; dout[4] = 0.5 * da4[2]; }
        else { dout[4] = 0.5 * da4[1]; dout[3] = 0.5 * da4[2]; }
    } else {
        dout[0] = da4[0]; dout[1] = da4[1]; dout[2] = da4[2]; dout[3] = da4[3];
    }
}

// For the Jacobian-vector product only: pair blockIdx.y's h, d-pre and d-out of sr_amp_factors_kernel once more, one thread per
// sample, the block evaluated in float64 from the same packed float32 weights (staged in LDS) and each factor rounded to float32
// once.  The
// float32 stage's d-out = [c == occ] - softmax and d-pre = W2^T d-out are cancelling sums: their errors are relative to the
// terms, not to the factor, which is what a product with a v that lives on one tensor is measured against (a Gram entry never
// is: sr_gram takes the stage's own factors, as before).  x is exact and stays.
__global__ __launch_bounds__(64) void sr_amp_factors64_kernel(const NetDims d, const float *__restrict__ w, const int64_t M,
                                                              const uint64_t *__restrict__ keys, const SrFactorOut F, const int raw) {
    __shared__ float rows[128 * naqs::amp_row_stride(2 * (MAXP - 1)) + 8];      // the pair's packed rows (Ha <= 128) and b2 [8]
    const int n = (int)blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int nin = n == 0 ? 1 : 2 * n, S = naqs::amp_row_stride(nin), Ha = d.Ha, nout = d.n_out_amp;
    for (int e = threadIdx.x; e < Ha * S + 8; e += 64) rows[e] = w[d.amp_off[n] + e];
    __syncthreads();
    if (i >= M) return;
    const float *b2 = rows + Ha * S;                       // packed row j: W1[j][:], b1[j], W2[:][j]
    const auto [abits, bbits, occ] = naqs::key_pair_view(d, n, keys[i]);
    const bool swap = (raw ? d.phase_sym != 0 : d.sym != 0) && abits > bbits;
    const uint32_t xb = n == 0 ? 0u : ((swap ? bbits : abits) | ((swap ? abits : bbits) << n));
    float *ho = F.h + ((int64_t)n * F.cap + i) * F.ldh, *dho = F.dh + ((int64_t)n * F.cap + i) * F.ldh;
    float *doo = F.dout + ((int64_t)n * F.cap + i) * XLD;
    double o[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, dout[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) if (c < nout) o[c] = b2[c];
    for (int j = 0; j < Ha; ++j) {
        const float *row = rows + j * S;
        double pre = row[nin];
        if (n > 0)                                         // (pair 0: the constant-zero input)
            for (int k = 0; k < nin; ++k) pre += ((xb >> k) & 1u) ? (double)row[k] : -(double)row[k];
        const double h = pre > 0.0 ? pre : 0.0;
        ho[j] = (float)h;
#pragma unroll
        for (int c = 0; c < 5; ++c) if (c < nout) o[c] += (double)row[nin + 1 + c] * h;
    }
    sr_block_delta64(d, n, raw != 0, o, abits, bbits, occ, dout);
#pragma unroll
    for (int c = 0; c < 5; ++c) doo[c] = (float)dout[c];
    for (int j = 0; j < Ha; ++j) {
        const float *row = rows + j * S + nin + 1;
        double dh = 0.0;
#pragma unroll
        for (int c = 0; c < 5; ++c) if (c < nout) dh += (double)row[c] * dout[c];
        dho[j] = ho[j] > 0.0f ? (float)dh : 0.0f;
    }
}

// acc[a][b] += F[I rows][0..K) . F[J rows][0..K)^T for this wave's 32 x 32 sub-block (2 x 2 MFMA tiles): 32-deep chunks of both
// row tiles staged in LDS as [64][CH] (rows >= M read as zero), the next chunk fetched while this one's MFMAs run.
// A operand: lane (m, q) holds Is[row m][k = q]; B operand: Js[row m][k = q], both widened to float64 (exact); the float64 form's
// D: col = lane & 15 (J), row = (lane >> 4) + 4 r (I) — not the float32 forms' map.
__device__ __forceinline__ void sr_tile_product(const float *__restrict__ Fm, const int ld, const int K, const int64_t M,
                                                const int64_t i0, const int64_t j0, float *Is, float *Js, f64x4 (&acc)[2][2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1, lm = lane & 15, lq = lane >> 4;
    f32x4 vi[2], vj[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + 256 * u, r = e >> 3, c4 = e & 7;
            vi[u] = (f32x4){0.f, 0.f, 0.f, 0.f}; vj[u] = vi[u];
            if (i0 + r < M) vi[u] = *reinterpret_cast<const f32x4 *>(Fm + (i0 + r) * ld + k0 + 4 * c4);
            if (j0 + r < M) vj[u] = *reinterpret_cast<const f32x4 *>(Fm + (j0 + r) * ld + k0 + 4 * c4);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += CH) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + 256 * u, r = e >> 3, c4 = e & 7;
            float2 *di = reinterpret_cast<float2 *>(Is + r * LDD + 4 * c4);       // LDD even: 8-byte aligned
            float2 *dj = reinterpret_cast<float2 *>(Js + r * LDD + 4 * c4);
            di[0] = make_float2(vi[u][0], vi[u][1]); di[1] = make_float2(vi[u][2], vi[u][3]);
            dj[0] = make_float2(vj[u][0], vj[u][1]); dj[1] = make_float2(vj[u][2], vj[u][3]);
        }
        __syncthreads();
        if (k0 + CH < K) fetch(k0 + CH);
#pragma unroll
        for (int ks = 0; ks < CH / 4; ++ks) {
            const int kk = ks * 4 + lq;
            const double a0 = Is[(wi * 32 + lm) * LDD + kk], a1 = Is[(wi * 32 + 16 + lm) * LDD + kk];
            const double b0 = Js[(wj * 32 + lm) * LDD + kk], b1 = Js[(wj * 32 + 16 + lm) * LDD + kk];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
}

// G[I, J] = sum_l (D_l D_l^T)[I, J] o ((A_l A_l^T)[I, J] + one_l), l in the jobs' order, for the tile (I = blockIdx.x,
// J = blockIdx.y >= I) and its transpose.  The whole feature axis of a factor is one workgroup's: no split, no second pass.
__global__ __launch_bounds__(256) void sr_gram_kernel(const SrJobs J, const int64_t M, double *__restrict__ G) {
    if (blockIdx.y < blockIdx.x) return;
    __shared__ __attribute__((aligned(16))) float Is[TB * LDD];
    __shared__ __attribute__((aligned(16))) float Js[TB * LDD];
    const int64_t i0 = (int64_t)blockIdx.x * TB, j0 = (int64_t)blockIdx.y * TB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = wave >> 1, wj = wave & 1, lm = lane & 15, lq = lane >> 4;
    double g[2][2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) g[a][b][r] = 0.0;
    for (int l = 0; l < J.n; ++l) {
        f64x4 pd[2][2], pa[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) { pd[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0}; pa[a][b] = pd[a][b]; }
        sr_tile_product(J.D[l], J.ldd[l], J.kd[l], M, i0, j0, Is, Js, pd);
        sr_tile_product(J.A[l], J.lda[l], J.ka[l], M, i0, j0, Is, Js, pa);
        const double one = J.one[l] ? 1.0 : 0.0;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) g[a][b][r] += pd[a][b][r] * (pa[a][b][r] + one);
    }
    const bool off_diag = blockIdx.y != blockIdx.x;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = i0 + wi * 32 + a * 16 + lq + 4 * r, j = j0 + wj * 32 + b * 16 + lm;
                if (i < M && j < M) {
                    G[i * M + j] = g[a][b][r];
                    if (off_diag) G[j * M + i] = g[a][b][r];
                }
            }
}

// part[y][i] = this workgroup's share of u_i = sum_l sum_j D_l[i][j] ((A_l V_l^T)[i][j] + one_l v_b,l[j]) for the 64 rows of tile
// blockIdx.x: the Jacobian-vector product (J v)_i of the block whose jobs these are, V_l and v_b,l read in place from the flat
// vector v through Vm (rows >= rows_l and columns >= cols_l read as zero; a job with one = 0 has its bias as column cols_l,
// where its A factor holds the ones).
// Per job and 64 columns j of D: P = A_tile V^T over 32-deep chunks with sr_tile_product's operand maps (wave (wi, wj): rows
// 32 wi.., columns 32 wj.. as 2 x 2 MFMA tiles; a 16-column tile past rows_l is skipped), then d (P + v_b) into the lane's
// eight row sums.  The sums over a row's 16 lanes (butterfly) and two waves (LDS, wave 0 first) come last: a fixed order in
// which row i meets nothing but row i's factors, so u_i has the same bits at any M that holds the row.
// A workgroup that walked every job alone would be a chain of ~190 staged chunks on N2 while M = 1 500 fills 24 of 256 CUs, so the
// (job, 64 columns) items are dealt round-robin to the gridDim.y workgroups of a tile (a count the host takes from the network
// alone, never from M) and sr_jvp_sum_kernel adds the partial sums in the order of y.
__global__ __launch_bounds__(256) void sr_jvp_kernel(const SrJobs J, const naqs::SrJvpMap Vm, const int64_t M,
                                                     const float *__restrict__ v, double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float Is[TB * LDD];
    __shared__ __attribute__((aligned(16))) float Js[TB * LDD];
    __shared__ double s_u[2][TB];
    const int y = (int)blockIdx.y, ny = (int)gridDim.y;
    int item = 0;
    const int64_t i0 = (int64_t)blockIdx.x * TB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1, lm = lane & 15, lq = lane >> 4;
    double us[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) us[a][r] = 0.0;
    for (int l = 0; l < J.n; ++l) {
        const float *__restrict__ Am = J.A[l], *__restrict__ Dm = J.D[l];
        const int lda = J.lda[l], ldd = J.ldd[l], ka = J.ka[l];
        const int N = Vm.rows[l], K = Vm.cols[l], ldw = Vm.ld[l];
        const float *__restrict__ Wv = v + Vm.w[l], *__restrict__ Bv = v + Vm.b[l];
        const bool one = J.one[l] != 0;
        for (int j0 = 0; j0 < N; j0 += TB) {
            if (item++ % ny != y) continue;                                      // (uniform over the workgroup)
            const bool act[2] = {j0 + wj * 32 < N, j0 + wj * 32 + 16 < N};       // wave-uniform
            f64x4 p[2][2];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) p[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
            f32x4 va[2];
            float vv[8];
            auto fetch = [&](int k0) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int e = tid + 256 * t, r = e >> 3, c4 = e & 7;
                    va[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if (i0 + r < M) va[t] = *reinterpret_cast<const f32x4 *>(Am + (i0 + r) * lda + k0 + 4 * c4);
                }
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const int e = tid + 256 * t, j = j0 + (e >> 5), k = k0 + (e & 31);
                    float x = 0.0f;
                    if (j < N) {
                        if (k < K) x = Wv[(int64_t)j * ldw + k];
                        else if (k == K && !one) x = Bv[j];
                    }
                    vv[t] = x;
                }
            };
            fetch(0);
            for (int k0 = 0; k0 < ka; k0 += CH) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int e = tid + 256 * t, r = e >> 3, c4 = e & 7;
                    float2 *di = reinterpret_cast<float2 *>(Is + r * LDD + 4 * c4);       // LDD even: 8-byte aligned
                    di[0] = make_float2(va[t][0], va[t][1]); di[1] = make_float2(va[t][2], va[t][3]);
                }
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const int e = tid + 256 * t;
                    Js[(e >> 5) * LDD + (e & 31)] = vv[t];
                }
                __syncthreads();
                if (k0 + CH < ka) fetch(k0 + CH);
#pragma unroll
                for (int ks = 0; ks < CH / 4; ++ks) {
                    const int kk = ks * 4 + lq;
                    const double a0 = Is[(wi * 32 + lm) * LDD + kk], a1 = Is[(wi * 32 + 16 + lm) * LDD + kk];
                    if (act[0]) {
                        const double b0 = Js[(wj * 32 + lm) * LDD + kk];
                        p[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, p[0][0], 0, 0, 0);
                        p[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, p[1][0], 0, 0, 0);
                    }
                    if (act[1]) {
                        const double b1 = Js[(wj * 32 + 16 + lm) * LDD + kk];
                        p[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, p[0][1], 0, 0, 0);
                        p[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, p[1][1], 0, 0, 0);
                    }
                }
                __syncthreads();
            }
            // the float64 form's D: column = lane & 15 (j), row = (lane >> 4) + 4 r (i)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int j = j0 + wj * 32 + b * 16 + lm;
                if (!act[b] || j >= N) continue;
                const double vb = one ? (double)Bv[j] : 0.0;
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t i = i0 + wi * 32 + a * 16 + lq + 4 * r;
                        if (i < M) us[a][r] += (double)Dm[i * ldd + j] * (p[a][b][r] + vb);
                    }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double t = us[a][r];
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
            if (lm == 0) s_u[wj][wi * 32 + a * 16 + lq + 4 * r] = t;
        }
    __syncthreads();
    if (tid < TB && i0 + tid < M) part[(int64_t)y * M + i0 + tid] = s_u[0][tid] + s_u[1][tid];
}

// the (job, 64 columns) items of a block's jobs, and the workgroups per tile they are dealt to
constexpr int JVP_SPLIT_MAX = 16;
inline int sr_jvp_split(const SrJobs &J, const naqs::SrJvpMap &Vm) {
    int items = 0;
    for (int l = 0; l < J.n; ++l) items += (Vm.rows[l] + TB - 1) / TB;
    return std::max(1, std::min(items, JVP_SPLIT_MAX));
}

// u_i = part[0][i] + part[1][i] + ... + part[ny - 1][i], in this order
__global__ __launch_bounds__(256) void sr_jvp_sum_kernel(const int64_t M, const int ny, const double *__restrict__ part,
                                                         double *__restrict__ u) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    double t = part[i];
    for (int y = 1; y < ny; ++y) t += part[(int64_t)y * M + i];
    u[i] = t;
}

// sum over the 256 threads of a workgroup in a fixed order (butterfly within a wave, the four waves added in order): every
// thread gets the same bits.  s_red: 4 doubles of LDS; ends with a barrier so that s_red can be used again.
__device__ __forceinline__ double block_sum_256(double v, double *s_red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    __syncthreads();
    return t;
}

// one wave per row i: m_i = sum_j G_ij w_j (lane-strided partial sums in ascending j, then the butterfly), the diagonal
// element, and the right-hand side y_i = g[i][col] / (2 sqrt w_i)
__global__ __launch_bounds__(256) void sr_rowsum_kernel(const int64_t M, const double *__restrict__ G, const double *__restrict__ w,
                                                        const float *__restrict__ g, const int col, double *__restrict__ m,
                                                        double *__restrict__ diag, double *__restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= M) return;
    const double *row = G + i * M;
    double v = 0.0;
    for (int64_t j = lane; j < M; j += 64) v += row[j] * w[j];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) {
        m[i] = v;
        diag[i] = row[i];
        y[i] = (double)g[2 * i + col] / (2.0 * sqrt(w[i]));
    }
}

// T = D (G - m 1^T - 1 m^T + c) D + lambda I in place, 16 rows per workgroup.  c = w^T G w = sum_i w_i m_i and the trace
// tr T = sum_i w_i (G_ii - 2 m_i + c) are formed by every workgroup itself from m, the saved diagonal and w, in the same
// fixed order: the same bits everywhere, and no launch or hand-over in between.
constexpr int CENTER_ROWS = 16;
__global__ __launch_bounds__(256) void sr_center_kernel(const int64_t M, double *__restrict__ G, const double *__restrict__ w,
                                                        const double *__restrict__ m, const double *__restrict__ diag,
                                                        const double diag_shift) {
    __shared__ double s_red[4];
    double s_wm = 0.0, s_wd = 0.0, s_w = 0.0;
    for (int64_t i = threadIdx.x; i < M; i += 256) {
        const double wi = w[i];
        s_wm += wi * m[i];
        s_wd += wi * diag[i];
        s_w += wi;
    }
    const double c = block_sum_256(s_wm, s_red);
    const double wd = block_sum_256(s_wd, s_red), ws = block_sum_256(s_w, s_red);
    const double lambda = diag_shift * (((wd - 2.0 * c) + c * ws) / (double)M);
    const int64_t r0 = (int64_t)blockIdx.x * CENTER_ROWS;
    for (int r = 0; r < CENTER_ROWS; ++r) {
        const int64_t i = r0 + r;
        if (i >= M) break;
        const double mi = m[i], si = sqrt(w[i]);
        double *row = G + i * M;
        for (int64_t j = threadIdx.x; j < M; j += 256) {
            const double t = si * (((row[j] - mi) - m[j]) + c) * sqrt(w[j]);
            row[j] = i == j ? t + lambda : t;
        }
    }
}

// s[i][col] = sqrt(w_i) x_i - w_i sum_j sqrt(w_j) x_j for both columns (x_a, x_phi), as float32 seeds for the backward pass;
// every workgroup forms the two sums itself, in the same fixed order
__global__ __launch_bounds__(256) void sr_seeds_kernel(const int64_t M, const double *__restrict__ w, const double *__restrict__ xa,
                                                       const double *__restrict__ xp, float2 *__restrict__ s) {
    __shared__ double s_red[4];
    double pa = 0.0, pp = 0.0;
    for (int64_t j = threadIdx.x; j < M; j += 256) {
        const double sq = sqrt(w[j]);
        pa += sq * xa[j];
        pp += sq * xp[j];
    }
    const double Sa = block_sum_256(pa, s_red), Sp = block_sum_256(pp, s_red);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const double wi = w[i], sq = sqrt(wi);
    s[i] = make_float2((float)(sq * xa[i] - wi * Sa), (float)(sq * xp[i] - wi * Sp));
}

// carve-up of net->d_sr for `cap` rows
struct SrLayout {
    size_t x[2], dout[2], h[2], dh[2];      // per block set: [P][cap][ld] floats
    size_t unit, seeds;                     // [cap][2] floats: the constant seeds (1, 1), the direction's seeds
    size_t m[2], diag[2];                   // [cap] doubles per Gram block
    size_t jvp_part;                        // [JVP_SPLIT_MAX][cap] doubles: sr_jvp_kernel's partial sums (one block at a time)
    int ldh[2];
    size_t total;
};

SrLayout sr_layout(const naqs_net *net, const int64_t cap) {
    SrLayout L{};
    size_t off = 0;
    const int n_sets = naqs::has_second_set(net) ? 2 : 1;
    for (int k = 0; k < n_sets; ++k) {
        const NetDims &d = k == 0 ? net->amp.d : net->ph.d;
        L.ldh[k] = pad64(d.Ha);
        const size_t thin = (size_t)d.P * cap * XLD * sizeof(float), wide = (size_t)d.P * cap * L.ldh[k] * sizeof(float);
        L.x[k] = off; off = up256(off + thin);
        L.dout[k] = off; off = up256(off + thin);
        L.h[k] = off; off = up256(off + wide);
        L.dh[k] = off; off = up256(off + wide);
    }
    L.unit = off; off = up256(off + (size_t)cap * 2 * sizeof(float));
    L.seeds = off; off = up256(off + (size_t)cap * 2 * sizeof(float));
    for (int k = 0; k < 2; ++k) {
        L.m[k] = off; off = up256(off + (size_t)cap * sizeof(double));
        L.diag[k] = off; off = up256(off + (size_t)cap * sizeof(double));
    }
    L.jvp_part = off; off = up256(off + (size_t)JVP_SPLIT_MAX * cap * sizeof(double));
    L.total = off;
    return L;
}

int ensure_sr_scratch(naqs_net *net, const int64_t M) {
    if (M <= net->sr_cap && net->d_sr) return NAQS_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (net->d_sr) (void)hipFree(net->d_sr);
    net->d_sr = nullptr; net->sr_cap = 0;
    const int64_t cap = std::min<int64_t>(naqs::SR_MAX_ROWS, std::max<int64_t>(1024, M + M / 4));
    const SrLayout L = sr_layout(net, cap);
    if (hipMalloc(&net->d_sr, L.total) != hipSuccess) { net->d_sr = nullptr; return NAQS_ERR_NOMEM; }
    HIP_TRY(hipMemset(net->d_sr, 0, L.total));             // the factors' padding columns stay zero for good
    HIP_TRY(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(static_cast<char *>(net->d_sr) + L.unit), 0x3f800000, (size_t)cap * 2));
    HIP_TRY(hipDeviceSynchronize());
    net->sr_cap = cap;
    return NAQS_OK;
}

// the per-pair factors of one block set and its jobs: pair n adds (d-out, h | +1) then (d-pre, x with the bias column); with `map`,
// where the two layers sit in the flat parameters (state_dict order per pair: W1 [Ha][nin], b1 [Ha], Wo [nout][Ha], bo [nout])
int sr_block_factors(naqs_net *net, const naqs::BlockSet &set, const int k, const SrLayout &L, const int64_t M,
                     const uint64_t *keys_dev, SrJobs *jobs, hipStream_t s, naqs::SrJvpMap *map = nullptr) {
    const NetDims &d = set.d;
    if (d.Ha > 128 || (d.Ha & 15) || set.deep() || 2 * d.P > naqs::SR_MAX_JOBS) return NAQS_ERR_UNSUPPORTED;
    const size_t lds = naqs::ampbw::smem_floats(d) * sizeof(float);
    if (lds > MAX_DYN_LDS) return NAQS_ERR_UNSUPPORTED;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&sr_amp_factors_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS));
    char *base = static_cast<char *>(net->d_sr);
    SrFactorOut F;
    F.x = reinterpret_cast<float *>(base + L.x[k]); F.dout = reinterpret_cast<float *>(base + L.dout[k]);
    F.h = reinterpret_cast<float *>(base + L.h[k]); F.dh = reinterpret_cast<float *>(base + L.dh[k]);
    F.cap = net->sr_cap; F.ldh = L.ldh[k];
    NAQS_KLAUNCH(sr_amp_factors_kernel, dim3((unsigned)naqs::ampbw::tile_wgs(M), (unsigned)d.P), dim3((unsigned)((d.Ha >> 4) * WAVE)), lds, s,
                       d, set.w, M, keys_dev, reinterpret_cast<const float *>(base + L.unit), F, set.raw ? 1 : 0);
    HIP_TRY(hipGetLastError());
    if (map) {                                            // the Jacobian-vector product: h, d-pre, d-out from a float64 evaluation
        NAQS_KLAUNCH(sr_amp_factors64_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)d.P), dim3(64), 0, s, d, set.w, M, keys_dev, F,
                     set.raw ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    jobs->n = 2 * d.P;
    const int kh = (d.Ha + 31) & ~31;
    for (int n = 0; n < d.P; ++n) {
        const int64_t thin = (int64_t)n * F.cap * XLD, wide = (int64_t)n * F.cap * F.ldh;
        jobs->D[2 * n] = F.dout + thin; jobs->ldd[2 * n] = XLD; jobs->kd[2 * n] = CH;
        jobs->A[2 * n] = F.h + wide; jobs->lda[2 * n] = F.ldh; jobs->ka[2 * n] = kh; jobs->one[2 * n] = 1;
        jobs->D[2 * n + 1] = F.dh + wide; jobs->ldd[2 * n + 1] = F.ldh; jobs->kd[2 * n + 1] = kh;
        jobs->A[2 * n + 1] = F.x + thin; jobs->lda[2 * n + 1] = XLD; jobs->ka[2 * n + 1] = CH; jobs->one[2 * n + 1] = 0;
        if (map) {
            const int nin = n == 0 ? 1 : 2 * n, nout = d.n_out_amp;
            const int64_t w1 = set.src_off[n], b1 = w1 + (int64_t)d.Ha * nin, wo = b1 + d.Ha, bo = wo + (int64_t)nout * d.Ha;
            map->w[2 * n] = wo; map->b[2 * n] = bo; map->ld[2 * n] = d.Ha; map->rows[2 * n] = nout; map->cols[2 * n] = d.Ha;
            map->w[2 * n + 1] = w1; map->b[2 * n + 1] = b1; map->ld[2 * n + 1] = nin; map->rows[2 * n + 1] = d.Ha; map->cols[2 * n + 1] = nin;
        }
    }
    return NAQS_OK;
}

// what both entry points refuse
int sr_supported(const naqs_net *net) {
    if (net->family == naqs::Family::COMBINED) return NAQS_ERR_UNSUPPORTED;       // W1 of the last block is shared between a and phi
    if (net->amp.deep() || net->ph.deep()) return NAQS_ERR_UNSUPPORTED;           // more than one hidden layer per block
    return NAQS_OK;
}

}  // namespace

// the per-layer factors of both blocks for unit seeds, into the handle's scratch: ja the amplitude block's jobs, jp the phase's
// (ma, mp: their layers' places in the flat parameters, for the Jacobian-vector product)
static int sr_factors(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, SrJobs *ja, SrJobs *jp, hipStream_t s,
                      naqs::SrJvpMap *ma = nullptr, naqs::SrJvpMap *mp = nullptr) {
    int st = ensure_sr_scratch(net, M);
    if (st != NAQS_OK) return st;
    const SrLayout L = sr_layout(net, net->sr_cap);
    char *base = static_cast<char *>(net->d_sr);
    st = sr_block_factors(net, net->amp, 0, L, M, keys_dev, ja, s, ma);
    if (st != NAQS_OK) return st;
    if (naqs::has_phase_mlp(net)) return naqs::net_sr_phase_factors(net, M, keys_dev, reinterpret_cast<const float *>(base + L.unit), jp, s, mp);
    return sr_block_factors(net, net->ph, 1, L, M, keys_dev, jp, s, mp);
}

// the factors and the two uncentred Gram matrices G_a -> T[0], G_phi -> T[1]
static int sr_gram_impl(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, double *const T[2], hipStream_t s) {
    int st = naqs::net_sr_begin(net, M, s);
    if (st != NAQS_OK) return st;
    SrJobs ja{}, jp{};
    st = sr_factors(net, M, keys_dev, &ja, &jp, s);
    if (st != NAQS_OK) return st;
    const unsigned nt = (unsigned)((M + TB - 1) / TB);
    NAQS_KLAUNCH(sr_gram_kernel, dim3(nt, nt), dim3(256), 0, s, ja, M, T[0]);
    HIP_TRY(hipGetLastError());
    NAQS_KLAUNCH(sr_gram_kernel, dim3(nt, nt), dim3(256), 0, s, jp, M, T[1]);
    HIP_TRY(hipGetLastError());
    return NAQS_OK;
}

NAQS_API int naqs_net_sr_gram_uncentred(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, double *Ga_dev, double *Gphi_dev,
                                        void *stream) {
    if (!net) return NAQS_ERR_INVALID;
    int st = sr_supported(net);
    if (st != NAQS_OK) return st;
    if (M < 1 || !keys_dev || !Ga_dev || !Gphi_dev) return NAQS_ERR_INVALID;
    if (M > naqs::SR_MAX_ROWS) return NAQS_ERR_UNSUPPORTED;
    DeviceGuard guard;
    st = guard.init(net->device);
    if (st != NAQS_OK) return st;
    double *const T[2] = {Ga_dev, Gphi_dev};
    return sr_gram_impl(net, M, keys_dev, T, reinterpret_cast<hipStream_t>(stream));
}

NAQS_API int naqs_net_sr_jvp(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, const float *v_dev, double *ua_dev, double *uphi_dev,
                             void *stream) {
    if (!net) return NAQS_ERR_INVALID;
    int st = sr_supported(net);
    if (st != NAQS_OK) return st;
    if (M < 1 || !keys_dev || !v_dev || !ua_dev || !uphi_dev) return NAQS_ERR_INVALID;
    if (M > naqs::SR_MAX_ROWS) return NAQS_ERR_UNSUPPORTED;
    DeviceGuard guard;
    st = guard.init(net->device);
    if (st != NAQS_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    st = naqs::net_sr_begin(net, M, s);
    if (st != NAQS_OK) return st;
    SrJobs j[2] = {};
    naqs::SrJvpMap m[2] = {};
    st = sr_factors(net, M, keys_dev, &j[0], &j[1], s, &m[0], &m[1]);
    if (st != NAQS_OK) return st;
    double *const u[2] = {ua_dev, uphi_dev};
    double *part = reinterpret_cast<double *>(static_cast<char *>(net->d_sr) + sr_layout(net, net->sr_cap).jvp_part);
    for (int k = 0; k < 2; ++k) {
        for (int l = 0; l < j[k].n; ++l) {                 // every layer inside v, and inside its factors' columns
            const int N = m[k].rows[l], K = m[k].cols[l];
            if (N < 1 || K < 1 || m[k].ld[l] < K || m[k].w[l] < 0 || m[k].w[l] + (int64_t)(N - 1) * m[k].ld[l] + K > net->n_params ||
                m[k].b[l] < 0 || m[k].b[l] + N > net->n_params || N > j[k].kd[l] || K + (j[k].one[l] ? 0 : 1) > j[k].ka[l])
                return NAQS_ERR_INVALID;
        }
        const int ny = sr_jvp_split(j[k], m[k]);
        NAQS_KLAUNCH(sr_jvp_kernel, dim3((unsigned)((M + TB - 1) / TB), (unsigned)ny), dim3(256), 0, s, j[k], m[k], M, v_dev, part);
        HIP_TRY(hipGetLastError());
        NAQS_KLAUNCH(sr_jvp_sum_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, M, ny, part, u[k]);
        HIP_TRY(hipGetLastError());
    }
    return NAQS_OK;
}

NAQS_API int naqs_net_sr_gram(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, const double *w_dev, const float *g_dev,
                              double diag_shift, double *Ta_dev, double *Tphi_dev, double *ya_dev, double *yphi_dev, void *stream) {
    if (!net) return NAQS_ERR_INVALID;
    int st = sr_supported(net);
    if (st != NAQS_OK) return st;
    if (M < 1 || !(diag_shift > 0.0) || !keys_dev || !w_dev || !g_dev || !Ta_dev || !Tphi_dev || !ya_dev || !yphi_dev) return NAQS_ERR_INVALID;
    if (M > naqs::SR_MAX_ROWS) return NAQS_ERR_UNSUPPORTED;
    DeviceGuard guard;
    st = guard.init(net->device);
    if (st != NAQS_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    double *const T[2] = {Ta_dev, Tphi_dev};
    double *const y[2] = {ya_dev, yphi_dev};
    st = sr_gram_impl(net, M, keys_dev, T, s);
    if (st != NAQS_OK) return st;
    const SrLayout L = sr_layout(net, net->sr_cap);
    char *base = static_cast<char *>(net->d_sr);
    for (int k = 0; k < 2; ++k) {
        double *m = reinterpret_cast<double *>(base + L.m[k]), *diag = reinterpret_cast<double *>(base + L.diag[k]);
        NAQS_KLAUNCH(sr_rowsum_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, M, T[k], w_dev, g_dev, k, m, diag, y[k]);
        HIP_TRY(hipGetLastError());
        NAQS_KLAUNCH(sr_center_kernel, dim3((unsigned)((M + CENTER_ROWS - 1) / CENTER_ROWS)), dim3(256), 0, s, M, T[k], w_dev, m, diag,
                           diag_shift);
        HIP_TRY(hipGetLastError());
    }
    return NAQS_OK;
}

NAQS_API int naqs_net_sr_direction(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, const double *w_dev, const double *xa_dev,
                                   const double *xphi_dev, float *dir_dev, void *stream) {
    if (!net) return NAQS_ERR_INVALID;
    int st = sr_supported(net);
    if (st != NAQS_OK) return st;
    if (M < 1 || !keys_dev || !w_dev || !xa_dev || !xphi_dev || !dir_dev) return NAQS_ERR_INVALID;
    if (M > naqs::SR_MAX_ROWS) return NAQS_ERR_UNSUPPORTED;
    DeviceGuard guard;
    st = guard.init(net->device);
    if (st != NAQS_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    st = naqs::net_sr_begin(net, M, s);
    if (st != NAQS_OK) return st;
    st = ensure_sr_scratch(net, M);
    if (st != NAQS_OK) return st;
    const SrLayout L = sr_layout(net, net->sr_cap);
    float *seeds = reinterpret_cast<float *>(static_cast<char *>(net->d_sr) + L.seeds);
    NAQS_KLAUNCH(sr_seeds_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, M, w_dev, xa_dev, xphi_dev,
                       reinterpret_cast<float2 *>(seeds));
    HIP_TRY(hipGetLastError());
    return naqs_net_train_backward(net, M, keys_dev, seeds, dir_dev, stream);
}
