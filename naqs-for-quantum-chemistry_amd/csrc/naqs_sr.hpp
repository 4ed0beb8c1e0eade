// naqs_sr.hpp — what the natural-gradient (minSR) entry points of naqs_sr.hip share with the training backward
// (naqs_phase_grad.hip): the geometry of the GEMM tiles, the factor pairs the Gram kernel walks, and the phase MLP's delta chain.
#pragma once
#include <cstdint>

#include "naqs_common.hpp"
#include "naqs_net.hpp"

namespace naqs {

// the LDS operand tile of the sample-axis GEMMs (grad_w_kernel, grad_in_kernel, sr_gram_kernel, sr_jvp_kernel) and the padding of their operands
// (each kernel's block edge TB stays with the kernel: the test suite reads the backward pass's from naqs_phase_grad.hip)
namespace bwtile {
constexpr int CH = 32;       // reduction chunk staged in LDS
constexpr int LDD = 34;      // row stride of a [64][CH] tile: bank = 2 row + k -> conflict-free for 16 rows x 2 k
inline int pad64(int x) { return (x + 63) & ~63; }
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
}  // namespace bwtile

// A Linear layer's per-sample gradient is delta_i (x) a_i, so the layer adds (D D^T) o (A A^T + 1) to the M x M Gram
// matrix of the per-sample gradients (`one`: the bias is not a column of A).  Factor l: D_l [M][ldd] and A_l [M][lda],
// row-major float32, of which the first kd / ka columns (multiples of 32, zero-padded) are read.
constexpr int SR_MAX_JOBS = 2 * MAXP;
struct SrJobs {
    int n;
    const float *D[SR_MAX_JOBS], *A[SR_MAX_JOBS];
    int ldd[SR_MAX_JOBS], lda[SR_MAX_JOBS], kd[SR_MAX_JOBS], ka[SR_MAX_JOBS], one[SR_MAX_JOBS];
};
// Where job l's Linear layer sits in a flat parameter-shaped vector v (state_dict order), for the Jacobian-vector product
// (sr_jvp_kernel): the weight V_l = v[w ...] as [rows][cols] with row stride ld (unpadded), the bias v_b = v[b ...] as [rows].
// rows is the true width of D_l, cols the true width of A_l; a job with one = 0 has the bias as column `cols` of V_l (where its A
// factor holds the ones).  Filled beside SrJobs, which stays as sr_gram_kernel takes it.
struct SrJvpMap {
    int64_t w[SR_MAX_JOBS], b[SR_MAX_JOBS];
    int ld[SR_MAX_JOBS], rows[SR_MAX_JOBS], cols[SR_MAX_JOBS];
};
constexpr int SR_MAX_ROWS = 32768;       // the Gram matrices are O(M^2) doubles: 8.6 GB each at this size

// naqs_phase_grad.hip.  net_sr_begin: naqs_net_train_backward's own readiness check (pending re-pack flushed, weights packed, the
// training forward's scratch holds M rows).  net_sr_phase_factors: the training backward's delta chain of the single phase MLP
// (phase_delta_chain) with the seeds unit_g [M][2] = (., 1), into the training scratch; the layers' (delta, input) pairs -> jobs,
// and with `map` where each layer's weight and bias sit in the flat parameters.
int net_sr_begin(naqs_net *net, int64_t M, hipStream_t s);
int net_sr_phase_factors(naqs_net *net, int64_t M, const uint64_t *keys_dev, const float *unit_g, SrJobs *jobs, hipStream_t s,
                         SrJvpMap *map = nullptr);

}  // namespace naqs
