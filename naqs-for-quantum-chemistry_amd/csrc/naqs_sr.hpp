// naqs_sr.hpp — what the natural-gradient (minSR) entry points of naqs_sr.hip share with the training backward
// (naqs_phase_grad.hip): the factor pairs the Gram kernel walks, and the host sequencing of the phase MLP's delta chain.
#pragma once
#include <cstdint>

#include "naqs_common.hpp"
#include "naqs_net.hpp"

namespace naqs {

// A Linear layer's per-sample gradient is delta_i (x) a_i, so the layer adds (D D^T) o (A A^T + 1) to the M x M Gram
// matrix of the per-sample gradients (`one`: the bias is not a column of A).  Factor l: D_l [M][ldd] and A_l [M][lda],
// row-major float32, of which the first kd / ka columns (multiples of 32, zero-padded) are read.
constexpr int SR_MAX_JOBS = 2 * MAXP;
struct SrJobs {
    int n;
    const float *D[SR_MAX_JOBS], *A[SR_MAX_JOBS];
    int ldd[SR_MAX_JOBS], lda[SR_MAX_JOBS], kd[SR_MAX_JOBS], ka[SR_MAX_JOBS], one[SR_MAX_JOBS];
};
constexpr int SR_MAX_ROWS = 32768;       // the Gram matrices are O(M^2) doubles: 8.6 GB each at this size

// naqs_phase_grad.hip.  net_sr_begin: what naqs_net_train_backward checks before it launches (pending re-pack flushed, weights
// packed, the training forward's scratch holds M rows).  net_sr_phase_factors: the unfused delta chain of the single phase MLP
// (top_delta_kernel -> delta_below_top_kernel -> grad_in_kernel) with the seeds unit_g [M][2] = (., 1), into the training
// scratch; the layers' (delta, input) pairs -> jobs.
int net_sr_begin(naqs_net *net, int64_t M, hipStream_t s);
int net_sr_phase_factors(naqs_net *net, int64_t M, const uint64_t *keys_dev, const float *unit_g, SrJobs *jobs, hipStream_t s);

}  // namespace naqs
