// naqs_amp_deep.hpp — amplitude blocks with 2..4 hidden layers of one width Ha (BlockSet::depth > 1): the weight
// layout, the forward evaluator for one (tile of 16 samples, pair) work item and the backward pass for one pair, shared by
// the standalone log-amplitude launch (naqs_logpsi.hip: amp_deep_kernel), the tree sampler (naqs_sample.hip:
// sample_expand_deep_kernel) and the gradient (naqs_grad.hip: amp_deep_backward_kernel).  gfx950 only.
//
// Every product runs on the f32 matrix cores (v_mfma_f32_16x16x4_f32), so there is no split format and no scale: the
// evaluator rounds like a float32 reference up to the order of its sums.  Layout of the operands, TRANSPOSED as in
// naqs_amp_mfma.hpp (the activations never leave the registers between layers):
//   layer 1   H^T [Ha x 16] = W1 [Ha x 2n] . X^T [2n x 16] + b1: A = W1 (lane (m, kq) reads W1[16 ot + m][4 kc + kq]),
//             B = the +-1 inputs (lane (s, kq) supplies input 4 kc + kq of sample s) -> D: lane (s, kq) holds units
//             16 ot + 4 kq + r of sample s.
//   layer l   H_l^T = W_l [Ha x Ha] . H_{l-1}^T + b_l: the contraction index in chunks (ct, r) = units {16 ct + 4 kq + r}:
//             lane (s, kq) supplies exactly its own register h[ct][r] as the B operand; A reads W_l[16 ot + m][16 ct + 4 kq + r]
//             (four r at once: one 16-byte load).
//   output    O^T [nout x 16] = Wo . H_L^T + bo the same way, rows m >= nout zero.
// The packed copy (deep_pack_kernel) is the state_dict of each pair, moved to a 16-byte aligned offset per pair (DeepAmp::off).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "naqs_net.hpp"

namespace naqs {

constexpr int MAX_AMP_LAYERS = 4;

// floats of pair n's parameters in state_dict order: W1 [Ha][nin], b1, (W_l [Ha][Ha], b_l) x (L - 1), Wo [nout][Ha], bo
__host__ __device__ inline int64_t deep_pair_floats(int Ha, int nout, int L, int n) {
    const int64_t nin = n == 0 ? 1 : 2 * n;
    return (int64_t)Ha * nin + Ha + (int64_t)(L - 1) * ((int64_t)Ha * Ha + Ha) + (int64_t)nout * Ha + nout;
}
// offsets inside a pair's block
__host__ __device__ inline int64_t deep_b1(int Ha, int n) { return (int64_t)Ha * (n == 0 ? 1 : 2 * n); }
__host__ __device__ inline int64_t deep_w(int Ha, int n, int l) {          // W_l, l = 1 .. L - 1 (hidden -> hidden)
    return deep_b1(Ha, n) + Ha + (int64_t)(l - 1) * ((int64_t)Ha * Ha + Ha);
}
__host__ __device__ inline int64_t deep_wo(int Ha, int n, int L) { return deep_w(Ha, n, L); }

struct DeepAmp {
    int32_t L = 1;                // hidden layers
    int64_t off[MAXP] = {};       // pair n's block in the packed copy (floats, multiples of 4)
    int64_t src[MAXP] = {};       // ... and in the flat source
};

// a deep block set's description of itself (kernel argument)
inline DeepAmp deep_blocks(const BlockSet &b) {
    DeepAmp a;
    a.L = b.depth;
    for (int n = 0; n < MAXP; ++n) { a.off[n] = b.deep_off[n]; a.src[n] = b.src_off[n]; }
    return a;
}

// The deep kernels are templates on CT = Ha / 16 in 1..8: f(std::integral_constant<int, CT>) for the runtime width, which launches
// and returns a status; any other width: NAQS_ERR_UNSUPPORTED, f not called.
template <typename F>
inline int dispatch_width(const int ct, F &&f) {
    switch (ct) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
        default: return NAQS_ERR_UNSUPPORTED;
    }
}

#if defined(__HIPCC__)

__device__ __forceinline__ f32x4 mfma4(float a, float b, const f32x4 &c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// max(x, 0) on a matrix-core result in one instruction (see relu1 in naqs_amp_mfma.hpp)
__device__ __forceinline__ float relu_i(float x) { return __int_as_float(max(__float_as_int(x), 0)); }

// +-1 input k of a pair-n block (k < 2n: the first n from `first`, the next n from `second`), 0 beyond
__device__ __forceinline__ float deep_input(int n, uint32_t first, uint32_t second, int k) {
    if (k >= 2 * n) return 0.0f;
    const uint32_t bit = k < n ? (first >> k) & 1u : (second >> (k - n)) & 1u;
    return bit ? 1.0f : -1.0f;
}

// layer 1 (pre-activation, bias included) of pair n for lane (s, kq)'s sample
template <int CT>
__device__ __forceinline__ void deep_layer1(const float *__restrict__ wp, int n, uint32_t first, uint32_t second, int lane,
                                            f32x4 (&h)[CT]) {
    constexpr int Ha = CT * 16;
    const int m = lane & 15, kq = lane >> 4;
    const int nin = n == 0 ? 1 : 2 * n;
    const float *b1 = wp + deep_b1(Ha, n);
#pragma unroll
    for (int ot = 0; ot < CT; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) h[ot][r] = b1[16 * ot + 4 * kq + r];
    const int kc_n = (2 * n + 3) >> 2;                      // pair 0: its one input is the constant 0 — no chunk
    for (int kc = 0; kc < kc_n; ++kc) {
        const int k = 4 * kc + kq;
        const float x = deep_input(n, first, second, k);
#pragma unroll
        for (int ot = 0; ot < CT; ++ot) {
            const float a = k < 2 * n ? wp[(16 * ot + m) * nin + k] : 0.0f;
            h[ot] = mfma4(a, x, h[ot]);
        }
    }
}

// y = W . relu(h) + b for a [rows x Ha] layer W at `wl` (rows = Ha: CT output tiles; the output layer: one tile, rows >= nout zero)
template <int CT, int OT>
__device__ __forceinline__ void deep_dense(const float *__restrict__ wl, int rows, int lane, const f32x4 (&h)[CT], f32x4 (&y)[OT]) {
    constexpr int Ha = CT * 16;
    const int m = lane & 15, kq = lane >> 4;
    const float *bl = wl + (int64_t)rows * Ha;
#pragma unroll
    for (int ot = 0; ot < OT; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * ot + 4 * kq + r;
            y[ot][r] = row < rows ? bl[row] : 0.0f;
        }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        f32x4 a[OT];
#pragma unroll
        for (int ot = 0; ot < OT; ++ot) {
            const int row = 16 * ot + m;
            a[ot] = row < rows ? *reinterpret_cast<const f32x4 *>(wl + (int64_t)row * Ha + 16 * ct + 4 * kq) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float b = relu_i(h[ct][r]);
#pragma unroll
            for (int ot = 0; ot < OT; ++ot) y[ot] = mfma4(a[ot][r], b, y[ot]);
        }
    }
}

// One wave, one (tile of 16 samples, pair n) item through all L hidden layers: the block's raw outputs -> outs[sample][8]
// (entries >= nout are 0).  ab: the occupation strings (alpha | beta << 16) of sample lane & 15.  wp: pair n's packed block.
// hs (optional): per hidden layer l the post-ReLU activations, hs[l - 1][unit * hs_ld + sample] (the backward pass).
// RAW: a phase block of an aggregate-phase network (d = net->ph.d): it orders its inputs under d.phase_sym, not d.sym.
template <int CT, bool RAW = false>
__device__ __forceinline__ void amp_deep_item(const NetDims &d, const float *__restrict__ wp, int L, int n, uint32_t ab, int lane,
                                              float *__restrict__ outs, float *hs = nullptr, int hs_ld = 0, int hs_layer = 0) {
    constexpr int Ha = CT * 16;
    const int s = lane & 15, kq = lane >> 4;
    const uint32_t mask = (1u << n) - 1u;
    const uint32_t abits = ab & mask, bbits = (ab >> 16) & mask;
    const bool swap = (RAW ? d.phase_sym : d.sym) && abits > bbits;             // nade.py:519-530
    const uint32_t first = swap ? bbits : abits, second = swap ? abits : bbits;
    f32x4 h[CT];
    deep_layer1<CT>(wp, n, first, second, lane, h);
    for (int l = 1; l <= L; ++l) {
        if (hs != nullptr) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) hs[(size_t)(l - 1) * hs_layer + (16 * ct + 4 * kq + r) * hs_ld + s] = relu_i(h[ct][r]);
        }
        if (l == L) break;
        f32x4 y[CT];
        deep_dense<CT, CT>(wp + deep_w(Ha, n, l), Ha, lane, h, y);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) h[ct] = y[ct];
    }
    f32x4 o[1];
    deep_dense<CT, 1>(wp + deep_wo(Ha, n, L), d.n_out_amp, lane, h, o);
    if (kq < 2) *reinterpret_cast<f32x4 *>(outs + s * 8 + 4 * kq) = o[0];
}
#endif

// ---- backward: one pair, all 64-sample tiles of this workgroup (4 waves; wave w runs the forward and the back-propagation of
// samples 16 w .. 16 w + 15 in registers, as above with W^T as the A operand).  What the weight gradients need goes through
// LDS: slot l - 1 of s_h holds h_l (post-ReLU) [unit][sample] until the gradient of the layer above has read it, then d pre_l.
// Each weight gradient is a GEMM with the tile's samples as K on the f32 matrix cores; its 16 x 16 tiles (plus one tile per row
// block whose only B column is the constant 1: the bias) are dealt to the waves round-robin, and every element is owned by one
// lane, which adds the tile's sum to the workgroup's partial in memory — a fixed order, no atomics.
constexpr int DGT = 64, DBW = 4;
__host__ __device__ inline size_t deep_bw_smem_floats(int Ha, int L) {
    return (size_t)L * Ha * (DGT + 1) + 8 * DGT + DGT + DBW * 128;
}

#if defined(__HIPCC__)
// out_w[j * ldo + k] (+)= sum_s A(j, s) B(k, s) for j < J, k < K; out_b[j] (+)= sum_s A(j, s)
template <typename FA, typename FB>
__device__ __forceinline__ void deep_gemm(int J, int K, FA fa, FB fb, float *__restrict__ out_w, int ldo, float *__restrict__ out_b,
                                          bool first, int lane, int wave) {
    const int m = lane & 15, kq = lane >> 4;
    const int JT = (J + 15) >> 4, KT = (K + 15) >> 4;
    for (int t = wave; t < JT * (KT + 1); t += DBW) {
        const int jt = t / (KT + 1), kt = t - jt * (KT + 1);
        const bool bias = kt == KT;
        const int j = 16 * jt + m, k = 16 * kt + m;
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int s0 = 0; s0 < DGT; s0 += 4) {
            const int sm = s0 + kq;
            const float a = j < J ? fa(j, sm) : 0.0f;
            const float b = bias ? (m == 0 ? 1.0f : 0.0f) : (k < K ? fb(k, sm) : 0.0f);
            acc = mfma4(a, b, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {                       // D: row = 4 kq + r (j), col = lane & 15 (k)
            const int jr = 16 * jt + 4 * kq + r;
            if (jr >= J) continue;
            float *dst = bias ? (m == 0 ? out_b + jr : nullptr) : (k < K ? out_w + (int64_t)jr * ldo + k : nullptr);
            if (dst != nullptr) *dst = first ? acc[r] : *dst + acc[r];
        }
    }
}

// RAW: a phase block of an aggregate-phase network (d = net->ph.d): d out[c] = g_i [c == phase_out_row(occ)], no conditional, and
// the inputs in phase_sym order (the depth-1 blocks' raw mode, naqs_amp_backward.hpp).  g_stride 2: a column of the loss gradient [M][2].
template <int CT, bool RAW = false>
__device__ __forceinline__ void amp_deep_backward_pair(const NetDims &d, const float *__restrict__ wp, const int L, const int n,
                                                       const int64_t M, const uint64_t *__restrict__ keys, const float *__restrict__ g,
                                                       float *__restrict__ out, float *smem, const int wg, const int n_wgs,
                                                       const int g_stride = 1) {
    constexpr int Ha = CT * 16, LD = DGT + 1;
    const int layer = Ha * LD, nout = d.n_out_amp, nin = n == 0 ? 1 : 2 * n;
    float *s_h = smem;                                                  // [L][Ha][LD]
    float *s_do = s_h + (size_t)L * layer;                              // [8][DGT] d outputs
    uint32_t *s_x = reinterpret_cast<uint32_t *>(s_do + 8 * DGT);      // [DGT] the block's inputs: first | second << 16
    float *s_outs = reinterpret_cast<float *>(s_x + DGT);              // [DBW][128] raw outputs
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), s = lane & 15, kq = lane >> 4, m = lane & 15;
    const int col = 16 * wave + s;                                      // this lane's sample in the tile
    const float *wo = wp + deep_wo(Ha, n, L);
    bool first_tile = true;
    for (int64_t t0 = (int64_t)wg * DGT; t0 < M; t0 += (int64_t)n_wgs * DGT) {
        const int64_t i = t0 + col;
        const bool valid = i < M;
        const uint64_t key = valid ? keys[i] : 0ull;
        const auto [abits, bbits, occ] = naqs::key_pair_view(d, n, key);
        float *outs = s_outs + wave * 128;
        amp_deep_item<CT, RAW>(d, wp, L, n, abits | (bbits << 16), lane, outs, s_h + 16 * wave, LD, layer);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (kq == 0) {                                      // lanes 0..15: d log-amp (RAW: d phase) / d outputs of their sample
            float o[5], dout[5];
#pragma unroll
            for (int c = 0; c < 5; ++c) o[c] = outs[s * 8 + c];
            naqs::amp_block_delta(d, n, RAW, o, abits, bbits, occ, valid, valid ? g[i * g_stride] : 0.0f, dout);
#pragma unroll
            for (int c = 0; c < 8; ++c) s_do[c * DGT + col] = c < 5 ? dout[c] : 0.0f;
            const bool swap = (RAW ? d.phase_sym : d.sym) && abits > bbits;
            s_x[col] = (swap ? bbits : abits) | ((swap ? abits : bbits) << 16);
        }
        __syncthreads();
        // d pre_L = [h_L > 0] Wo^T d out, in registers
        f32x4 dp[CT];
#pragma unroll
        for (int ot = 0; ot < CT; ++ot) dp[ot] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            const int c = 4 * kc + kq;
            const float b = s_do[c * DGT + col];
#pragma unroll
            for (int ot = 0; ot < CT; ++ot) dp[ot] = mfma4(c < nout ? wo[c * Ha + 16 * ot + m] : 0.0f, b, dp[ot]);
        }
#pragma unroll
        for (int ot = 0; ot < CT; ++ot)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (!(s_h[(size_t)(L - 1) * layer + (16 * ot + 4 * kq + r) * LD + col] > 0.0f)) dp[ot][r] = 0.0f;
        // d Wo, d bo = d out . h_L^T
        {
            const float *hl = s_h + (size_t)(L - 1) * layer;
            deep_gemm(nout, Ha, [&](int j, int sm) { return s_do[j * DGT + sm]; }, [&](int k, int sm) { return hl[k * LD + sm]; },
                      out + deep_wo(Ha, n, L), Ha, out + deep_wo(Ha, n, L) + (int64_t)nout * Ha, first_tile, lane, wave);
        }
        __syncthreads();
#pragma unroll
        for (int ot = 0; ot < CT; ++ot)
#pragma unroll
            for (int r = 0; r < 4; ++r) s_h[(size_t)(L - 1) * layer + (16 * ot + 4 * kq + r) * LD + col] = dp[ot][r];
        for (int l = L; l >= 2; --l) {
            // d pre_{l-1} = [h_{l-1} > 0] W^T d pre_l, W = the layer h_{l-1} -> h_l
            const float *W = wp + deep_w(Ha, n, l - 1);
            f32x4 nd[CT];
#pragma unroll
            for (int ot = 0; ot < CT; ++ot) nd[ot] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float *wr = W + (int64_t)(16 * ct + 4 * kq + r) * Ha + m;
#pragma unroll
                    for (int ot = 0; ot < CT; ++ot) nd[ot] = mfma4(wr[16 * ot], dp[ct][r], nd[ot]);
                }
            const float *hprev = s_h + (size_t)(l - 2) * layer;
#pragma unroll
            for (int ot = 0; ot < CT; ++ot)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (!(hprev[(16 * ot + 4 * kq + r) * LD + col] > 0.0f)) nd[ot][r] = 0.0f;
            __syncthreads();                                // every wave's d pre_l is in slot l - 1
            {
                const float *dpl = s_h + (size_t)(l - 1) * layer;
                float *gw = out + deep_w(Ha, n, l - 1);
                deep_gemm(Ha, Ha, [&](int j, int sm) { return dpl[j * LD + sm]; }, [&](int k, int sm) { return hprev[k * LD + sm]; },
                          gw, Ha, gw + (int64_t)Ha * Ha, first_tile, lane, wave);
            }
            __syncthreads();                                // ... and h_{l-1} has been read
#pragma unroll
            for (int ot = 0; ot < CT; ++ot) {
                dp[ot] = nd[ot];
#pragma unroll
                for (int r = 0; r < 4; ++r) s_h[(size_t)(l - 2) * layer + (16 * ot + 4 * kq + r) * LD + col] = nd[ot][r];
            }
        }
        __syncthreads();
        // d W1, d b1 = d pre_1 . x^T
        deep_gemm(Ha, nin, [&](int j, int sm) { return s_h[j * LD + sm]; },
                  [&](int k, int sm) { const uint32_t xb = s_x[sm]; return deep_input(n, xb & 0xFFFFu, xb >> 16, k); },
                  out, nin, out + (int64_t)Ha * nin, first_tile, lane, wave);
        __syncthreads();                                    // (the next tile rewrites every LDS array)
        first_tile = false;
    }
}
#endif

}  // namespace naqs
