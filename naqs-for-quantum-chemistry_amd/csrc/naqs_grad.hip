// naqs_grad.hip — training-time evaluation of the amplitude half of the orbital NADE on gfx950 (MI355X):
//   naqs_net_logamp        log|psi|(key_i) = sum_n [conditional log-amplitude of the realised outcome of pair n]
//   naqs_net_amp_backward  d/d theta  sum_i g_i log|psi|(key_i)  for every amplitude-block parameter
// i.e. the forward and backward of the amplitude part of _forward_predict (src/naqs/network/nade.py:738-770 with the
// helpers :417-630, activations.py:40-46) that the reference leaves to PyTorch autograd (energy.py:329-343).  The eager
// formulation is ~10 orbital pairs x (2 Linear + mask + softmax + gathers), forward and backward; here it is two
// kernels each way, and the gradient is deterministic (fixed-order reductions, no float atomics).
//
// amp_backward_kernel: workgroup = one orbital pair n (blockIdx.y) x a strided set of 256-sample tiles.  Per tile every
// thread owns a sample: it recomputes the block's forward from the key bits (weights staged in LDS), forms
// d log-amp / d outputs (softmax residual through the symmetrisation, nade.py:585-586) scaled by g_i and
// back-propagates to the hidden pre-activations.  The per-sample factors go through one LDS tile [hidden][sample];
// the threads then re-partition over the PARAMETERS (thread = hidden unit j x a subset of input columns) and walk
// the tile's samples, accumulating dW1, db1 (from d pre) and dW2, db2 (from h) in registers across all tiles of the
// workgroup.  Partial sums per workgroup go to scratch in state_dict order; amp_reduce_kernel adds them in order.

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdint>

#include "naqs_common.hpp"
#include "naqs_net.hpp"
#include "naqs_amp_deep.hpp"
#include "naqs_amp_backward.hpp"

namespace {

using naqs::MAXP;
using naqs::NetDims;
using naqs::WAVE;
using naqs::DeviceGuard;
typedef float f32x4 __attribute__((ext_vector_type(4)));

using naqs::ampbw::MAX_TILE_WGS;
using naqs::ampbw::AmpSrc;
using naqs::ampbw::MAX_DYN_LDS;

// out[i] = sum_n scratch[n][i] in the order of the fused log-psi epilogue
__global__ __launch_bounds__(256) void logamp_sum_kernel(int P, int64_t M, const float *__restrict__ scratch,
                                                         float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    float s = 0.0f;
    for (int n = 0; n < P; ++n) s += scratch[(int64_t)n * M + i];
    out[i] = s;
}

__global__ __launch_bounds__(512) void amp_backward_kernel(const NetDims d, const float *__restrict__ w, const int64_t M,
                                                           const uint64_t *__restrict__ keys, const float *__restrict__ g,
                                                           float *__restrict__ partial, const int64_t partial_stride,
                                                           const AmpSrc src, const int raw) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = blockIdx.y;
    float *out = partial + (int64_t)blockIdx.x * partial_stride + src.off[n];
    naqs::ampbw::pair_dispatch(n, d, w, M, keys, g, out, smem, raw, (int)blockIdx.x, (int)gridDim.x);
}

// deep amplitude blocks (naqs_net_create_amp_layers): workgroup = pair blockIdx.y x a strided set of 64-sample tiles, partial sums
// per workgroup in state_dict order like amp_backward_kernel's (naqs_amp_deep.hpp: amp_deep_backward_pair)
template <int CT>
__global__ __launch_bounds__(naqs::DBW * 64) void amp_deep_backward_kernel(const NetDims d, const float *__restrict__ wdeep, const naqs::DeepAmp da,
                                                                         const int64_t M, const uint64_t *__restrict__ keys,
                                                                         const float *__restrict__ g, float *__restrict__ partial,
                                                                         const int64_t partial_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = blockIdx.y;
    float *out = partial + (int64_t)blockIdx.x * partial_stride + (da.src[n] - da.src[0]);
    naqs::amp_deep_backward_pair<CT>(d, wdeep + da.off[n], da.L, n, M, keys, g, out, smem, (int)blockIdx.x, (int)gridDim.x);
}

// aggregate phase with deep blocks (naqs_net_create_agg_layers): the phase blocks (raw, d = net->ph.d) on g with stride g_stride, the
// same partial-sum layout
template <int CT>
__global__ __launch_bounds__(naqs::DBW * 64) void amp_deep_backward_raw_kernel(const NetDims d, const float *__restrict__ wdeep,
                                                                             const naqs::DeepAmp da, const int64_t M,
                                                                             const uint64_t *__restrict__ keys, const float *__restrict__ g,
                                                                             const int g_stride, float *__restrict__ partial,
                                                                             const int64_t partial_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = blockIdx.y;
    float *out = partial + (int64_t)blockIdx.x * partial_stride + (da.src[n] - da.src[0]);
    naqs::amp_deep_backward_pair<CT, true>(d, wdeep + da.off[n], da.L, n, M, keys, g, out, smem, (int)blockIdx.x, (int)gridDim.x, g_stride);
}

// ... and both sets in ONE launch when Ha == Hp: the amplitude blocks (blockIdx.z == 0, on g[:, 0]) and the phase blocks (1, raw,
// on g[:, 1]), the loss gradient read in place (stride 2); each into its half of the partial-sum scratch
template <int CT>
__global__ __launch_bounds__(naqs::DBW * 64) void agg_deep_backward_kernel(const NetDims d0, const float *__restrict__ w0, const naqs::DeepAmp da0,
                                                                         float *__restrict__ partial0, const NetDims d1,
                                                                         const float *__restrict__ w1, const naqs::DeepAmp da1,
                                                                         float *__restrict__ partial1, const int64_t M,
                                                                         const uint64_t *__restrict__ keys, const float *__restrict__ g_amp,
                                                                         const float *__restrict__ g_ph, const int g_stride,
                                                                         const int64_t partial_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = blockIdx.y;
    if (blockIdx.z == 0)
        naqs::amp_deep_backward_pair<CT, false>(d0, w0 + da0.off[n], da0.L, n, M, keys, g_amp,
                                                partial0 + (int64_t)blockIdx.x * partial_stride + (da0.src[n] - da0.src[0]), smem,
                                                (int)blockIdx.x, (int)gridDim.x, g_stride);
    else
        naqs::amp_deep_backward_pair<CT, true>(d1, w1 + da1.off[n], da1.L, n, M, keys, g_ph,
                                               partial1 + (int64_t)blockIdx.x * partial_stride + (da1.src[n] - da1.src[0]), smem,
                                               (int)blockIdx.x, (int)gridDim.x, g_stride);
}

// aggregate_phase: the amplitude blocks (blockIdx.z == 0, on g[:, 0]) and the per-pair phase blocks (1, raw, on g[:, 1]) in ONE
// launch; the loss gradient's two columns are read in place (stride 2), no split launch in front
// (the two sets' descriptions are separate kernel arguments: nested in a struct their dynamically indexed tables end up in
// scratch memory — measured 2x slower than two launches)
__global__ __launch_bounds__(512) void amp_backward2_kernel(const NetDims d0, const float *__restrict__ w0, float *__restrict__ partial0,
                                                            const AmpSrc src0, const NetDims d1, const float *__restrict__ w1,
                                                            float *__restrict__ partial1, const AmpSrc src1, const int64_t M,
                                                            const uint64_t *__restrict__ keys, const float *__restrict__ g_amp,
                                                            const float *__restrict__ g_ph, const int64_t partial_stride,
                                                            const int g_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = blockIdx.y;
    if (blockIdx.z == 0)
        naqs::ampbw::pair_dispatch(n, d0, w0, M, keys, g_amp, partial0 + (int64_t)blockIdx.x * partial_stride + src0.off[n], smem, 0,
                                   (int)blockIdx.x, (int)gridDim.x, g_stride);
    else
        naqs::ampbw::pair_dispatch(n, d1, w1, M, keys, g_ph, partial1 + (int64_t)blockIdx.x * partial_stride + src1.off[n], smem, 1,
                                   (int)blockIdx.x, (int)gridDim.x, g_stride);
}

// combined amplitude-phase blocks (naqs_net_create_combined): the amplitude blocks (blockIdx.y < P, on g[:, 0]) and the phase head
// (blockIdx.y == P: pair P - 1 of d1, raw, on g[:, 1]) in ONE launch; per workgroup the partial sums of both in the layout of
// net->d_cflat (amplitude blocks in the plain layout, the head at head_off)
__global__ __launch_bounds__(512) void comb_backward_kernel(const NetDims d0, const float *__restrict__ w0, const AmpSrc src0,
                                                            const NetDims d1, const float *__restrict__ w1, const int64_t head_off,
                                                            const int64_t M, const uint64_t *__restrict__ keys, const float *__restrict__ g,
                                                            const int g_stride, float *__restrict__ partial, const int64_t partial_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = blockIdx.y;
    float *out = partial + (int64_t)blockIdx.x * partial_stride;
    if (n < d0.P)
        naqs::ampbw::pair_dispatch(n, d0, w0, M, keys, g, out + src0.off[n], smem, 0, (int)blockIdx.x, (int)gridDim.x, g_stride);
    else
        naqs::ampbw::pair_dispatch(d1.P - 1, d1, w1, M, keys, g + 1, out + head_off, smem, 1, (int)blockIdx.x, (int)gridDim.x, g_stride);
}

// ... and the gradient in the flat layout: element e sums its amplitude partials, then (with_head) its head partials, each over the
// workgroups in order, and adds the two (the last block's W1 / b1 have both; naqs::comb_src); with a.p also Adam's update of e
__global__ __launch_bounds__(256) void comb_grad_finish_kernel(const naqs::CombLayout c, const int n_partials, const int64_t partial_stride,
                                                               const float *__restrict__ partial, const int with_head,
                                                               float *__restrict__ grad, const naqs::AdamArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= c.total) return;
    int64_t pa, ph;
    naqs::comb_src(c, e, pa, ph);
    float ga = 0.0f, gh = 0.0f;
    if (pa >= 0)
        for (int b = 0; b < n_partials; ++b) ga += partial[(int64_t)b * partial_stride + pa];
    if (ph >= 0 && with_head)
        for (int b = 0; b < n_partials; ++b) gh += partial[(int64_t)b * partial_stride + c.amp + ph];
    const float gi = pa >= 0 && ph >= 0 && with_head ? ga + gh : (pa >= 0 ? ga : gh);
    grad[e] = gi;
    if (a.p != nullptr) naqs::adam_update(a, e, gi);
}

__global__ __launch_bounds__(256) void amp_reduce_kernel(int64_t count, int n_partials, int64_t partial_stride,
                                                         const float *__restrict__ partial, float *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    float s = 0.0f;
    for (int b = 0; b < n_partials; ++b) s += partial[(int64_t)b * partial_stride + e];
    out[e] = s;
}

// inputs of the phase block from key bits: x[i][c] = +-1 occupation of (alpha of model pairs 0..P-2 | beta of the same),
// occ[i] = realised outcome of the last pair (selects the phase output, nade.py:563-569)
__global__ __launch_bounds__(256) void phase_inputs_kernel(const NetDims d, const int64_t M, const uint64_t *__restrict__ keys,
                                                           float *__restrict__ x, int64_t *__restrict__ occ) {
    const int W = 2 * (d.P - 1);
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= M * W) return;
    const int64_t i = e / W;
    const int c = (int)(e - i * W);
    const uint64_t key = keys[i];
    if (d.phase_sym) {                                  // spin-ordered inputs; occ = the row of the 3-output layer (naqs_net.hpp)
        uint32_t a_, b_;
        naqs::key_strings(d, key, a_, b_);
        naqs::phase_order_inputs(d, d.P - 1, a_, b_);
        x[e] = (c < d.P - 1 ? ((a_ >> c) & 1u) : ((b_ >> (c - (d.P - 1))) & 1u)) ? 1.0f : -1.0f;
    } else {
        const int bit = c < d.P - 1 ? d.qa[c] : d.qb[c - (d.P - 1)];
        x[e] = ((key >> bit) & 1ull) ? 1.0f : -1.0f;
    }
    if (c == 0) occ[i] = naqs::phase_out_row(d, (int)((key >> d.qa[d.P - 1]) & 1ull) + 2 * (int)((key >> d.qb[d.P - 1]) & 1ull));
}

// d loss / d (log|psi|, phase) of the VMC loss 2 Re sum_i w_i log psi_i (E_loc_i - <E>)^* in the reference's float32
// arithmetic (energy.py:328-329 with complex.py:49-58): g = (2 w Re(E_loc - <E>), -2 w Im(E_loc - <E>))
__global__ __launch_bounds__(256) void vmc_grad_kernel(const int64_t M, const double2 *__restrict__ eloc,
                                                       const double *__restrict__ w, const double *__restrict__ sums,
                                                       float2 *__restrict__ g, double *__restrict__ ev) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ev != nullptr && i == 0) {                     // <E> and Var of energy.py:372-375 from the same accumulators
        const double e_mean = sums[0] / sums[3];
        ev[0] = e_mean;
        ev[1] = sums[2] / sums[3] - e_mean * e_mean;
    }
    if (i >= M) return;
    const float m_re = (float)sums[0], m_im = (float)sums[1];
    const double2 e = eloc[i];
    const float two_w = 2.0f * (float)w[i];
    g[i] = make_float2(((float)e.x - m_re) * two_w, -(((float)e.y - m_im) * two_w));
}

// Adam on one flat parameter vector (naqs::adam_update, naqs_net.hpp)
__global__ __launch_bounds__(256) void adam_kernel(const int64_t n, const float *__restrict__ g, const naqs::AdamArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    naqs::adam_update(a, i, g[i]);
}

// the amp kernel of naqs_logpsi.hip is reached through naqs::net_amp_forward
}  // namespace

NAQS_API int naqs_adam_step(int64_t n, float *param_dev, const float *grad_dev, float *exp_avg_dev, float *exp_avg_sq_dev,
                            double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                            void *stream) {
    if (n < 0 || step < 1 || (n > 0 && (!param_dev || !grad_dev || !exp_avg_dev || !exp_avg_sq_dev))) return NAQS_ERR_INVALID;
    if (n == 0) return NAQS_OK;
    NAQS_KLAUNCH(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), n, grad_dev,
                       naqs::adam_args(param_dev, exp_avg_dev, exp_avg_sq_dev, lr, beta1, beta2, eps, weight_decay, step));
    HIP_TRY(hipGetLastError());
    return NAQS_OK;
}

NAQS_API int naqs_net_phase_inputs(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, float *x_dev, int64_t *occ_dev,
                                   void *stream) {
    if (!net || M < 0 || (M > 0 && (!keys_dev || !x_dev || !occ_dev))) return NAQS_ERR_INVALID;
    if (M == 0) return NAQS_OK;
    DeviceGuard guard;
    int st = guard.init(net->device);
    if (st != NAQS_OK) return st;
    const int64_t total = M * 2 * (net->amp.d.P - 1);
    NAQS_KLAUNCH(phase_inputs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       net->amp.d, M, keys_dev, x_dev, occ_dev);
    HIP_TRY(hipGetLastError());
    return NAQS_OK;
}

static int vmc_loss_grad_impl(int64_t M, const double *eloc_dev, const double *w_dev, const double *sums_dev, float *g_dev,
                              double *ev_dev, void *stream) {
    if (M < 0 || (M > 0 && (!eloc_dev || !w_dev || !sums_dev || !g_dev))) return NAQS_ERR_INVALID;
    if (M == 0 && ev_dev == nullptr) return NAQS_OK;
    if (!sums_dev) return NAQS_ERR_INVALID;
    NAQS_KLAUNCH(vmc_grad_kernel, dim3((unsigned)std::max<int64_t>(1, (M + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), M, reinterpret_cast<const double2 *>(eloc_dev), w_dev, sums_dev,
                       reinterpret_cast<float2 *>(g_dev), ev_dev);
    HIP_TRY(hipGetLastError());
    return NAQS_OK;
}

NAQS_API int naqs_vmc_loss_grad(int64_t M, const double *eloc_dev, const double *w_dev, const double *sums_dev, float *g_dev,
                                void *stream) {
    return vmc_loss_grad_impl(M, eloc_dev, w_dev, sums_dev, g_dev, nullptr, stream);
}

NAQS_API int naqs_vmc_loss_grad_ev(int64_t M, const double *eloc_dev, const double *w_dev, const double *sums_dev, float *g_dev,
                                   double *ev_dev, void *stream) {
    if (!ev_dev) return NAQS_ERR_INVALID;
    return vmc_loss_grad_impl(M, eloc_dev, w_dev, sums_dev, g_dev, ev_dev, stream);
}

namespace {
__global__ __launch_bounds__(1024) void shard_proof_kernel(const int64_t M, const uint64_t *__restrict__ keys,
                                                           const double *__restrict__ sums, double *__restrict__ ext) {
    __shared__ unsigned long long s_part[16];
    unsigned long long acc = 0ull;
    for (int64_t i = threadIdx.x; i < M; i += 1024) acc += keys[i];          // modulo 2^64: order-independent
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0ull;
        for (int w = 0; w < 16; ++w) t += s_part[w];
        const double c = (double)(t & 0xFFFFFull), m = (double)M;
        ext[0] = sums[0]; ext[1] = sums[1]; ext[2] = sums[2]; ext[3] = sums[3];
        ext[4] = m; ext[5] = m * m; ext[6] = c; ext[7] = c * c;
    }
}
}  // namespace

NAQS_API int naqs_shard_proof(int64_t M, const uint64_t *keys_dev, const double *sums_dev, double *ext_dev, void *stream) {
    if (M < 0 || (M > 0 && !keys_dev) || !sums_dev || !ext_dev) return NAQS_ERR_INVALID;
    NAQS_KLAUNCH(shard_proof_kernel, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), M, keys_dev, sums_dev, ext_dev);
    HIP_TRY(hipGetLastError());
    return NAQS_OK;
}

NAQS_API int naqs_net_amp_param_count(const naqs_net_t *net, int64_t *count) {
    if (!net || !count) return NAQS_ERR_INVALID;
    *count = net->amp.n_params;
    return NAQS_OK;
}

NAQS_API int naqs_net_logamp(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, float *logamp_dev, void *stream) {
    if (!net || M < 0 || (M > 0 && (!keys_dev || !logamp_dev))) return NAQS_ERR_INVALID;
    if (!net->have_amp_weights) return NAQS_ERR_INVALID;
    if (M == 0) return NAQS_OK;
    DeviceGuard guard;
    int st = guard.init(net->device);
    if (st != NAQS_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    st = naqs::net_flush_amp_pack(net, s);                 // (a training step's re-pack still waiting for a launch to host it)
    if (st != NAQS_OK) return st;
    st = naqs::net_amp_forward(net, M, keys_dev, s);
    if (st != NAQS_OK) return st;
    NAQS_KLAUNCH(logamp_sum_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, net->amp.d.P, M, net->d_scratch,
                       logamp_dev);
    HIP_TRY(hipGetLastError());
    return NAQS_OK;
}

// the two halves of the partial-sum scratch, one per block set that may be pending (allocated on first use): `slot`'s half
static int blocks_partials(naqs_net *net, const int slot, int64_t *stride, float **gpart) {
    *stride = (std::max(net->amp.n_params, net->ph.n_params) + 3) & ~3ll;
    if (!net->d_gpart) HIP_TRY(hipMalloc((void **)&net->d_gpart, 2 * (size_t)MAX_TILE_WGS * *stride * sizeof(float)));
    *gpart = net->d_gpart + (slot ? (size_t)MAX_TILE_WGS * *stride : 0);
    return NAQS_OK;
}

// gradient of sum_i g_i f(key_i) for one set of per-pair blocks (amplitude blocks: f = log|psi|; a raw set: the phase blocks
// of an aggregate-phase network, f = phase): partial sums per workgroup, then a fixed-order reduction
int naqs::net_blocks_backward(naqs_net *net, const BlockSet &set, int64_t M, const uint64_t *keys_dev, const float *g_dev, float *grad_dev,
                              hipStream_t s, BlockReduceJob *defer, int slot) {
    const NetDims &d = set.d;
    if (d.Ha > 128 || (d.Ha & 15)) return NAQS_ERR_UNSUPPORTED;                 // a wave owns 16-unit hidden tiles
    if (M == 0) {
        if (defer) return NAQS_ERR_INVALID;
        HIP_TRY(hipMemsetAsync(grad_dev, 0, (size_t)set.n_params * sizeof(float), s));
        return NAQS_OK;
    }
    const int n_wg = naqs::ampbw::tile_wgs(M);
    int64_t stride;
    float *gpart;
    int st = blocks_partials(net, slot, &stride, &gpart);
    if (st != NAQS_OK) return st;
    if (set.deep()) {
        const size_t lds_d = naqs::deep_bw_smem_floats(d.Ha, set.depth) * sizeof(float);
        if (lds_d > MAX_DYN_LDS) return NAQS_ERR_UNSUPPORTED;
        const naqs::DeepAmp da = naqs::deep_blocks(set);
        st = naqs::dispatch_width(d.Ha >> 4, [&](auto c) -> int {
            constexpr int C = decltype(c)::value;
            if (set.raw) {                                  // deep phase blocks
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&amp_deep_backward_raw_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS));
                NAQS_KLAUNCH(amp_deep_backward_raw_kernel<C>, dim3((unsigned)n_wg, (unsigned)d.P), dim3(naqs::DBW * WAVE), lds_d, s, d, set.w, da, M,
                             keys_dev, g_dev, 1, gpart, stride);
            } else {                                        // deep amplitude blocks
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&amp_deep_backward_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS));
                NAQS_KLAUNCH(amp_deep_backward_kernel<C>, dim3((unsigned)n_wg, (unsigned)d.P), dim3(naqs::DBW * WAVE), lds_d, s, d, set.w, da, M,
                             keys_dev, g_dev, gpart, stride);
            }
            HIP_TRY(hipGetLastError());
            return NAQS_OK;
        });
        if (st != NAQS_OK) return st;
        if (set.raw)
            std::snprintf(net->last_deep, sizeof(net->last_deep), "backward: amp_deep_backward_kernel<%d, L=%d> + amp_deep_backward_raw_kernel<%d, L=%d>",
                          net->amp.d.Ha >> 4, net->amp.depth, d.Ha >> 4, set.depth);
        else
            std::snprintf(net->last_deep, sizeof(net->last_deep), "backward: amp_deep_backward_kernel<%d, L=%d>", d.Ha >> 4, set.depth);
    } else {
        const int NW = d.Ha >> 4;
        const size_t lds = naqs::ampbw::smem_floats(d) * sizeof(float);
        if (lds > MAX_DYN_LDS) return NAQS_ERR_UNSUPPORTED;
        if (!net->grad_attr_set) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&amp_backward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS));
            net->grad_attr_set = true;
        }
        NAQS_KLAUNCH(amp_backward_kernel, dim3((unsigned)n_wg, (unsigned)d.P), dim3((unsigned)(NW * WAVE)), lds, s, d, set.w, M, keys_dev,
                           g_dev, gpart, stride, naqs::block_src<AmpSrc>(set, /*relative=*/true), set.raw ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    if (defer) {
        defer->count = set.n_params; defer->stride = stride; defer->n_partials = n_wg; defer->partial = gpart;
        return NAQS_OK;
    }
    NAQS_KLAUNCH(amp_reduce_kernel, dim3((unsigned)((set.n_params + 255) / 256)), dim3(256), 0, s, set.n_params, n_wg,
                       stride, gpart, grad_dev);
    HIP_TRY(hipGetLastError());
    return NAQS_OK;
}

// what net_blocks_backward would launch, for a caller that runs the workgroups inside a launch of its own
// (naqs_phase_grad.hip: backward_mega_kernel): the partial-sum scratch, the reduction it needs afterwards and the pairs' offsets
int naqs::net_blocks_backward_plan(naqs_net *net, const BlockSet &set, int64_t M, int slot, BlockReduceJob *job, naqs::ampbw::AmpSrc *src) {
    const NetDims &d = set.d;
    if (d.Ha > 128 || (d.Ha & 15) || M <= 0 || !job || !src) return NAQS_ERR_INVALID;
    if (set.deep()) return NAQS_ERR_UNSUPPORTED;           // (deep blocks: net_blocks_backward's own launch)
    int64_t stride;
    float *gpart;
    const int st = blocks_partials(net, slot, &stride, &gpart);
    if (st != NAQS_OK) return st;
    job->count = set.n_params; job->stride = stride; job->n_partials = naqs::ampbw::tile_wgs(M);
    job->partial = gpart;
    *src = naqs::block_src<AmpSrc>(set, /*relative=*/true);
    return NAQS_OK;
}

// both block sets of an aggregate-phase network in one launch (same hidden width and pair count); the reductions are left
// to the caller like net_blocks_backward's with `defer`
int naqs::net_blocks_backward2(naqs_net *net, int64_t M, const uint64_t *keys_dev, const float *g_amp, const float *g_ph, int g_stride,
                               BlockReduceJob jobs[2], hipStream_t s) {
    const NetDims &d0 = net->amp.d, &d1 = net->ph.d;
    if (d0.Ha != d1.Ha || d0.P != d1.P || M <= 0) return NAQS_ERR_INVALID;
    if (net->amp.deep()) {                        // deep blocks (naqs_net_create_agg_layers): agg_deep_backward_kernel, same partials
        if (d0.Ha > 128 || (d0.Ha & 15) || net->family != naqs::Family::AGGREGATE) return NAQS_ERR_UNSUPPORTED;
        const int n_wg = naqs::ampbw::tile_wgs(M);
        const size_t lds_d = naqs::deep_bw_smem_floats(d0.Ha, net->amp.depth) * sizeof(float);
        jobs[0].count = net->amp.n_params; jobs[1].count = net->ph.n_params;
        for (int k = 0; k < 2; ++k) {
            float *gpart;
            const int stp = blocks_partials(net, k, &jobs[k].stride, &gpart);
            if (stp != NAQS_OK) return stp;
            jobs[k].n_partials = n_wg; jobs[k].partial = gpart;
        }
        if (lds_d > MAX_DYN_LDS) return NAQS_ERR_UNSUPPORTED;
        const int64_t stride = jobs[0].stride;
        const naqs::DeepAmp da0 = naqs::deep_blocks(net->amp), da1 = naqs::deep_blocks(net->ph);
        const int st = naqs::dispatch_width(d0.Ha >> 4, [&](auto c) -> int {
            constexpr int C = decltype(c)::value;
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&agg_deep_backward_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS));
            NAQS_KLAUNCH(agg_deep_backward_kernel<C>, dim3((unsigned)n_wg, (unsigned)d0.P, 2), dim3(naqs::DBW * WAVE), lds_d, s, d0, net->amp.w, da0,
                         const_cast<float *>(jobs[0].partial), d1, net->ph.w, da1, const_cast<float *>(jobs[1].partial), M, keys_dev, g_amp, g_ph,
                         g_stride, stride);
            HIP_TRY(hipGetLastError());
            return NAQS_OK;
        });
        if (st != NAQS_OK) return st;
        std::snprintf(net->last_deep, sizeof(net->last_deep), "backward: agg_deep_backward_kernel<%d, L=%d>", d0.Ha >> 4, net->amp.depth);
        return NAQS_OK;
    }
    AmpSrc src0, src1;
    int st = net_blocks_backward_plan(net, net->amp, M, 0, &jobs[0], &src0);
    if (st != NAQS_OK) return st;
    st = net_blocks_backward_plan(net, net->ph, M, 1, &jobs[1], &src1);
    if (st != NAQS_OK) return st;
    const size_t lds = std::max(naqs::ampbw::smem_floats(d0), naqs::ampbw::smem_floats(d1)) * sizeof(float);
    if (lds > MAX_DYN_LDS) return NAQS_ERR_UNSUPPORTED;
    if (!net->grad2_attr_set) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&amp_backward2_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS));
        net->grad2_attr_set = true;
    }
    NAQS_KLAUNCH(amp_backward2_kernel, dim3((unsigned)jobs[0].n_partials, (unsigned)d0.P, 2), dim3((unsigned)((d0.Ha >> 4) * WAVE)), lds, s,
                       d0, net->amp.w, const_cast<float *>(jobs[0].partial), src0, d1, net->ph.w, const_cast<float *>(jobs[1].partial), src1, M,
                       keys_dev, g_amp, g_ph, jobs[0].stride, g_stride);
    HIP_TRY(hipGetLastError());
    return NAQS_OK;
}

int naqs::net_comb_backward(naqs_net *net, int64_t M, const uint64_t *keys_dev, const float *g_dev, int g_stride, bool with_head,
                             float *grad_dev, const naqs::AdamArgs *adam, hipStream_t s) {
    const NetDims &d0 = net->amp.d, &d1 = net->ph.d;
    if (net->family != naqs::Family::COMBINED || d0.Ha > 128 || (d0.Ha & 15) || d1.Ha != d0.Ha || d1.P != d0.P) return NAQS_ERR_UNSUPPORTED;
    if (M <= 0) {
        if (adam) return NAQS_ERR_INVALID;
        HIP_TRY(hipMemsetAsync(grad_dev, 0, (size_t)net->n_params * sizeof(float), s));
        return NAQS_OK;
    }
    const int n_wg = naqs::ampbw::tile_wgs(M);
    const int64_t stride = (net->comb_amp + net->comb_head + 3) & ~3ll;
    if (!net->d_cpart) HIP_TRY(hipMalloc((void **)&net->d_cpart, (size_t)MAX_TILE_WGS * stride * sizeof(float)));
    const size_t lds = std::max(naqs::ampbw::smem_floats(d0), naqs::ampbw::smem_floats(d1)) * sizeof(float);
    if (lds > MAX_DYN_LDS) return NAQS_ERR_UNSUPPORTED;
    if (!net->comb_attr_set) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&comb_backward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS));
        net->comb_attr_set = true;
    }
    const AmpSrc src = naqs::block_src<AmpSrc>(net->amp, /*relative=*/true);
    NAQS_KLAUNCH(comb_backward_kernel, dim3((unsigned)n_wg, (unsigned)(d0.P + (with_head ? 1 : 0))), dim3((unsigned)((d0.Ha >> 4) * WAVE)), lds, s,
                       d0, net->amp.w, src, d1, net->ph.w, net->comb_amp, M, keys_dev, g_dev, g_stride, net->d_cpart, stride);
    HIP_TRY(hipGetLastError());
    const naqs::CombLayout c = naqs::comb_layout(net);
    NAQS_KLAUNCH(comb_grad_finish_kernel, dim3((unsigned)((c.total + 255) / 256)), dim3(256), 0, s, c, n_wg, stride, net->d_cpart,
                       with_head ? 1 : 0, grad_dev, adam ? *adam : naqs::AdamArgs{});
    HIP_TRY(hipGetLastError());
    return NAQS_OK;
}

NAQS_API int naqs_net_amp_backward(naqs_net_t *net, int64_t M, const uint64_t *keys_dev, const float *g_dev,
                                   float *grad_dev, void *stream) {
    if (!net || M < 0 || !grad_dev || (M > 0 && (!keys_dev || !g_dev))) return NAQS_ERR_INVALID;
    if (!net->have_amp_weights) return NAQS_ERR_INVALID;
    DeviceGuard guard;
    int st = guard.init(net->device);
    if (st != NAQS_OK) return st;
    st = naqs::net_flush_amp_pack(net, reinterpret_cast<hipStream_t>(stream));
    if (st != NAQS_OK) return st;
    // combined blocks: log|psi| only — the phase rows get zero gradient, the flat layout is the whole parameter vector's
    if (net->family == naqs::Family::COMBINED)
        return naqs::net_comb_backward(net, M, keys_dev, g_dev, 1, false, grad_dev, nullptr, reinterpret_cast<hipStream_t>(stream));
    return naqs::net_blocks_backward(net, net->amp, M, keys_dev, g_dev, grad_dev, reinterpret_cast<hipStream_t>(stream));
}
