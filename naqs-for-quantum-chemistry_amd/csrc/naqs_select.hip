// naqs_select.hip — naqs_ham_pt2_select: which external states of a PT2 call join the subspace (selected CI).
//
// The rule (include/naqs_hip.h states it in full): eps_a = num_a^2 / (diag_a - e0), +inf for an intruder; tau = the k-th largest
// eligible eps; every eligible row with eps >= tau (1 - tie_rtol) is selected, in row order.  A non-negative double's bit pattern
// orders as the double does (+inf on top), so tau comes from an exact MSB-first radix select on 64-bit keys, 8 bits a pass, and
// a row that is not eligible has key 0 (an eligible eps is > 0, so its key is too).
//
// House rules: integer atomics only (LDS histograms, merged into global memory by integer atomics — the
// result does not depend on their order); no workgroup waits for another: every launch re-derives the digits chosen so far from
// the merged histograms, the compaction's offsets come from a counts launch and a one-workgroup scan; trip and launch counts
// depend on n_ext alone (all eight passes always run, whatever k); nothing is read back.  The one host synchronisation is the
// scratch's growth (form MULTI, when a call has more tiles than any before it on the handle), as naqs_ham_pt2 grows its rows.
//
// Two forms.  ONE: a single 1 024-thread workgroup does the eight passes and the ordered compaction in one launch, histograms
// in LDS only, no scratch.  MULTI: tiles of 2 048 rows, one 256-thread workgroup each; a memset, eight histogram launches, a
// counts launch, a one-workgroup scan and the scatter.  The crossover is measured (tools/sci_bench.py, profiles/sci.txt).
//
// naqs_ham_pt2_select_avg (selected CI for several roots) is the same call with another importance: the kernels
// that read rows are templates on their argument struct, and only row_key differs between SelArgs and SelAvgArgs.  The SelArgs
// instances have the device code they had before they were templates (tools/kernel_asm_diff.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "naqs_common.hpp"

using namespace naqs;

namespace {

constexpr int ONE_BLOCK = 1024;
constexpr int MULTI_BLOCK = 256;
constexpr int MULTI_ROWS = 8;
constexpr int MULTI_TILE = MULTI_BLOCK * MULTI_ROWS;     // 2 048 rows a workgroup
constexpr int DIGITS = 8, BINS = 256;
constexpr int HIST_WORDS = DIGITS * BINS + 8;            // [DIGITS][BINS] and, at DIGITS * BINS, the number of eligible rows

enum : int { MODE_NONE = 0, MODE_ALL = 1, MODE_CUT = 2 };

struct SelArgs {
    int64_t n;
    const uint64_t *keys;
    const double *num, *diag;
    double e0, eps_min, factor;      // factor = 1 - tie_rtol, formed on the host
    int64_t k;
    int64_t capacity;
    uint64_t *out;
    int64_t *count;
};

// eps of one row and its sort key (0: not eligible)
__device__ __forceinline__ uint64_t row_key(const SelArgs &a, const int64_t i, double *eps, bool *intruder) {
    const double num = a.num[i], den = a.diag[i] - a.e0;
    const bool intr = !(den > 0) || num != num;
    const double e = intr ? __builtin_inf() : (num * num) / den;
    *eps = e;
    *intruder = intr;
    return (e > 0 && e >= a.eps_min) ? (uint64_t)__double_as_longlong(e) : 0ull;
}

// naqs_ham_pt2_select_avg: the same call with the importances of several roots averaged.  Only the live roots (w != 0) travel,
// in ascending order: their columns of num [nb][n], energies and weights.  Every field the kernels share with SelArgs has its name.
constexpr int MAX_ROOTS = 8;
struct SelAvgArgs {
    int64_t n;
    const uint64_t *keys;
    const double *num, *diag;        // num [nb][n]
    double e[MAX_ROOTS], w[MAX_ROOTS];
    int32_t col[MAX_ROOTS], n_live;
    double eps_min, factor;
    int64_t k;
    int64_t capacity;
    uint64_t *out;
    int64_t *count;
};

// eps_a = w_0 q_0 + w_1 q_1 + ... over the live roots in order, q_j = (num_ja * num_ja) / (diag_a - e_j), each operation one
// rounding (the library is compiled without contraction); an intruder of ANY live root makes the row one
__device__ __forceinline__ uint64_t row_key(const SelAvgArgs &a, const int64_t i, double *eps, bool *intruder) {
    const double dg = a.diag[i];
    bool intr = false;
    double e = 0.0;
#pragma unroll
    for (int j = 0; j < MAX_ROOTS; ++j) {
        if (j >= a.n_live) break;
        const double num = a.num[(size_t)a.col[j] * (size_t)a.n + i], den = dg - a.e[j];
        intr = intr || !(den > 0) || num != num;
        const double t = a.w[j] * ((num * num) / den);
        e = j == 0 ? t : e + t;
    }
    if (intr) e = __builtin_inf();
    *eps = e;
    *intruder = intr;
    return (e > 0 && e >= a.eps_min) ? (uint64_t)__double_as_longlong(e) : 0ull;
}

// Wave 0: the digit that holds the k-th largest of a 256-bin histogram (k in 1 .. the histogram's total), and k within that bin.
// Lane l owns bins 4 l .. 4 l + 3; a suffix scan over the lanes by shuffles, no LDS, no barrier.  Every lane returns the result.
template <typename H>
__device__ __forceinline__ void pick_digit(const H *hist, uint32_t *k, uint32_t *digit) {
    const int lane = threadIdx.x & (WAVE - 1);
    const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
    const uint32_t tot = h0 + h1 + h2 + h3;
    uint32_t sfx = tot;
    for (int off = 1; off < WAVE; off <<= 1) {
        const uint32_t o = __shfl_down(sfx, off);
        if (lane + off < WAVE) sfx += o;
    }
    const uint32_t above = sfx - tot, kk = *k;
    uint32_t d = 0, kn = 0;
    const bool mine = above < kk && kk <= sfx;
    if (mine) {
        uint32_t acc = above;
        if (acc + h3 >= kk) { d = 4 * lane + 3; kn = kk - acc; }
        else if ((acc += h3) + h2 >= kk) { d = 4 * lane + 2; kn = kk - acc; }
        else if ((acc += h2) + h1 >= kk) { d = 4 * lane + 1; kn = kk - acc; }
        else { acc += h1; d = 4 * lane; kn = kk - acc; }
    }
    const unsigned long long who = __ballot(mine);
    const int src = who ? __ffsll((long long)who) - 1 : 0;       // exactly one lane when 1 <= k <= total
    *digit = __shfl(d, src);
    *k = __shfl(kn, src);
}

__device__ __forceinline__ uint32_t clamp_k(const int64_t k, const int64_t n) {
    return (uint32_t)(k < 1 ? 1 : (k > n ? n : k));
}

__device__ __forceinline__ int select_mode(const int64_t k, const int64_t n_elig) {
    return (k <= 0 || n_elig == 0) ? MODE_NONE : (k >= n_elig ? MODE_ALL : MODE_CUT);
}

__device__ __forceinline__ bool is_selected(const int mode, const uint64_t key, const double eps, const double cut) {
    return key != 0 && (mode == MODE_ALL || (mode == MODE_CUT && eps >= cut));
}

// Ordered append of one chunk of blockDim.x consecutive rows: -> this thread's position in the chunk and the chunk's total.
// Two barriers; s_w holds one word per wave.
__device__ __forceinline__ void chunk_offsets(const bool flag, uint32_t *s_w, uint32_t *pos, uint32_t *total) {
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE, nw = blockDim.x / WAVE;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) s_w[wv] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < nw; ++w) {
        const uint32_t c = s_w[w];
        before += w < wv ? c : 0;
        all += c;
    }
    __syncthreads();
    *pos = before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    *total = all;
}

// ---- form ONE ----------------------------------------------------------------------------------------------------------------
template <typename A>
__global__ __launch_bounds__(ONE_BLOCK) void select_one_kernel(const A a) {
    __shared__ uint32_t s_hist[BINS];
    __shared__ uint32_t s_w[ONE_BLOCK / WAVE];
    __shared__ uint32_t s_pick[2], s_elig, s_intr;
    const int t = threadIdx.x;
    uint64_t prefix = 0;
    uint32_t k = clamp_k(a.k, a.n);
    if (t == 0) { s_elig = 0; s_intr = 0; }
    for (int p = 0; p < DIGITS; ++p) {
        const int shift = 64 - 8 * (p + 1);
        if (t < BINS) s_hist[t] = 0;
        __syncthreads();
        uint32_t n_el = 0;
        for (int64_t i = t; i < a.n; i += ONE_BLOCK) {
            double eps;
            bool intr;
            const uint64_t key = row_key(a, i, &eps, &intr);
            n_el += key != 0;
            if (p == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&s_hist[(key >> shift) & 0xff], 1u);
        }
        if (p == 0 && n_el) atomicAdd(&s_elig, n_el);
        __syncthreads();
        if (t < WAVE) {
            uint32_t d, kk = k;
            pick_digit(s_hist, &kk, &d);
            if (t == 0) { s_pick[0] = d; s_pick[1] = kk; }
        }
        __syncthreads();
        prefix = (prefix << 8) | s_pick[0];
        k = s_pick[1];
    }
    const int mode = select_mode(a.k, (int64_t)s_elig);
    const double cut = __longlong_as_double((long long)prefix) * a.factor;
    uint32_t base = 0, n_intr = 0;
    for (int64_t i0 = 0; i0 < a.n; i0 += ONE_BLOCK) {
        const int64_t i = i0 + t;
        bool sel = false, intr = false;
        if (i < a.n) {
            double eps;
            const uint64_t key = row_key(a, i, &eps, &intr);
            sel = is_selected(mode, key, eps, cut);
        }
        uint32_t pos, total;
        chunk_offsets(sel, s_w, &pos, &total);
        if (sel) {
            n_intr += intr;
            if ((int64_t)(base + pos) < a.capacity) a.out[base + pos] = a.keys[i];
        }
        base += total;
    }
    if (n_intr) atomicAdd(&s_intr, n_intr);
    __syncthreads();
    if (t == 0) { a.count[0] = (int64_t)base; a.count[1] = (int64_t)s_intr; }
}

// ---- form MULTI --------------------------------------------------------------------------------------------------------------
// Wave 0 of every workgroup: the first `passes` digits from the merged histograms -> prefix, the k left inside it.
__device__ __forceinline__ void derive_prefix(const uint32_t *ghist, const int passes, const int64_t k_in, const int64_t n, uint64_t *prefix,
                                              uint32_t *k_left) {
    uint32_t k = clamp_k(k_in, n);
    uint64_t pre = 0;
    for (int q = 0; q < passes; ++q) {
        uint32_t d;
        pick_digit(ghist + q * BINS, &k, &d);
        pre = (pre << 8) | d;
    }
    *prefix = pre;
    *k_left = k;
}

// pass p: rows whose key starts with the prefix of passes 0 .. p-1 into hist[p]
template <typename A>
__global__ __launch_bounds__(MULTI_BLOCK) void select_hist_kernel(const A a, uint32_t *ghist, const int p) {
    __shared__ uint32_t s_hist[BINS];
    __shared__ unsigned long long s_prefix;
    __shared__ uint32_t s_elig;
    const int t = threadIdx.x;
    s_hist[t] = 0;                                   // MULTI_BLOCK == BINS
    if (t == 0) s_elig = 0;
    if (t < WAVE) {
        uint64_t pre;
        uint32_t kl;
        derive_prefix(ghist, p, a.k, a.n, &pre, &kl);
        if (t == 0) s_prefix = pre;
    }
    __syncthreads();
    const uint64_t prefix = s_prefix;
    const int shift = 64 - 8 * (p + 1);
    const int64_t base = (int64_t)blockIdx.x * MULTI_TILE;
    uint32_t n_el = 0;
#pragma unroll
    for (int r = 0; r < MULTI_ROWS; ++r) {
        const int64_t i = base + r * MULTI_BLOCK + t;
        if (i < a.n) {
            double eps;
            bool intr;
            const uint64_t key = row_key(a, i, &eps, &intr);
            n_el += key != 0;
            if (p == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&s_hist[(key >> shift) & 0xff], 1u);
        }
    }
    if (p == 0 && n_el) atomicAdd(&s_elig, n_el);
    __syncthreads();
    const uint32_t c = s_hist[t];
    if (c) atomicAdd(&ghist[p * BINS + t], c);
    if (p == 0 && t == 0 && s_elig) atomicAdd(&ghist[DIGITS * BINS], s_elig);
}

// the cut of a call, from the eight merged histograms (wave 0) -> LDS
template <typename A>
__device__ __forceinline__ void derive_cut(const A &a, const uint32_t *ghist, double *s_cut, int *s_mode) {
    if (threadIdx.x < WAVE) {
        uint64_t pre;
        uint32_t kl;
        derive_prefix(ghist, DIGITS, a.k, a.n, &pre, &kl);
        if (threadIdx.x == 0) {
            *s_cut = __longlong_as_double((long long)pre) * a.factor;
            *s_mode = select_mode(a.k, (int64_t)ghist[DIGITS * BINS]);
        }
    }
    __syncthreads();
}

// selected rows and selected intruders of every tile
template <typename A>
__global__ __launch_bounds__(MULTI_BLOCK) void select_count_kernel(const A a, const uint32_t *ghist, uint32_t *wg_cnt, uint32_t *wg_intr) {
    __shared__ double s_cut;
    __shared__ int s_mode;
    __shared__ uint32_t s_n[2];
    const int t = threadIdx.x;
    if (t == 0) { s_n[0] = 0; s_n[1] = 0; }
    derive_cut(a, ghist, &s_cut, &s_mode);
    const double cut = s_cut;
    const int mode = s_mode;
    const int64_t base = (int64_t)blockIdx.x * MULTI_TILE;
    uint32_t n_sel = 0, n_intr = 0;
#pragma unroll
    for (int r = 0; r < MULTI_ROWS; ++r) {
        const int64_t i = base + r * MULTI_BLOCK + t;
        if (i < a.n) {
            double eps;
            bool intr;
            const uint64_t key = row_key(a, i, &eps, &intr);
            const bool sel = is_selected(mode, key, eps, cut);
            n_sel += sel;
            n_intr += sel && intr;
        }
    }
    if (n_sel) atomicAdd(&s_n[0], n_sel);
    if (n_intr) atomicAdd(&s_n[1], n_intr);
    __syncthreads();
    if (t == 0) { wg_cnt[blockIdx.x] = s_n[0]; wg_intr[blockIdx.x] = s_n[1]; }
}

// one workgroup: exclusive scan of the tiles' counts -> wg_off; the two totals -> count
__global__ __launch_bounds__(ONE_BLOCK) void select_scan_kernel(const int64_t n_wg, const uint32_t *wg_cnt, const uint32_t *wg_intr, uint32_t *wg_off,
                                                                int64_t *count) {
    __shared__ uint32_t s_w[ONE_BLOCK / WAVE];
    __shared__ uint32_t s_intr;
    const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    if (t == 0) s_intr = 0;
    uint32_t base = 0, n_intr = 0;
    for (int64_t b0 = 0; b0 < n_wg; b0 += ONE_BLOCK) {
        const int64_t b = b0 + t;
        const uint32_t c = b < n_wg ? wg_cnt[b] : 0;
        n_intr += b < n_wg ? wg_intr[b] : 0;
        uint32_t inc = c;                                             // inclusive scan inside the wave
        for (int off = 1; off < WAVE; off <<= 1) {
            const uint32_t o = __shfl_up(inc, off);
            if (lane >= off) inc += o;
        }
        if (lane == WAVE - 1) s_w[wv] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int w = 0; w < ONE_BLOCK / WAVE; ++w) {
            const uint32_t x = s_w[w];
            before += w < wv ? x : 0;
            all += x;
        }
        __syncthreads();
        if (b < n_wg) wg_off[b] = base + before + inc - c;
        base += all;
    }
    if (n_intr) atomicAdd(&s_intr, n_intr);
    __syncthreads();
    if (t == 0) { count[0] = (int64_t)base; count[1] = (int64_t)s_intr; }
}

template <typename A>
__global__ __launch_bounds__(MULTI_BLOCK) void select_scatter_kernel(const A a, const uint32_t *ghist, const uint32_t *wg_off) {
    __shared__ double s_cut;
    __shared__ int s_mode;
    __shared__ uint32_t s_w[MULTI_BLOCK / WAVE];
    const int t = threadIdx.x;
    derive_cut(a, ghist, &s_cut, &s_mode);
    const double cut = s_cut;
    const int mode = s_mode;
    const int64_t base = (int64_t)blockIdx.x * MULTI_TILE;
    int64_t at = (int64_t)wg_off[blockIdx.x];
    for (int r = 0; r < MULTI_ROWS; ++r) {
        const int64_t i = base + r * MULTI_BLOCK + t;
        bool sel = false;
        if (i < a.n) {
            double eps;
            bool intr;
            const uint64_t key = row_key(a, i, &eps, &intr);
            sel = is_selected(mode, key, eps, cut);
        }
        uint32_t pos, total;
        chunk_offsets(sel, s_w, &pos, &total);
        if (sel && at + pos < a.capacity) a.out[at + pos] = a.keys[i];
        at += total;
    }
}

// One workgroup against the multi-workgroup form (NAQS_SELECT_FORM = 0).  Measured on one MI355X (tools/sci_bench.py sweep, HIP
// events around 20 back-to-back calls, three rounds; profiles/sci.txt, section 3): form ONE costs 11.5 us at 512 rows and 3.9 us per
// further 1 024 (25.8 us at 4 096, 41.5 at 8 192, 73.1 at 16 384: one workgroup's nine walks over the rows), form MULTI 48.3 us at
// 512 and 65 .. 69 us from 4 096 to 65 536 (its eleven launches), 90 us at 2^20.  ONE is ahead by 9.5 us at 12 288 rows, by 2 us
// (the rounds' spread) at 14 336, behind by 5.5 us at 16 384.
constexpr int64_t ONE_MAX_ROWS = 12288;

// the launches of one call, for either argument struct (the checks are the callers')
template <typename A>
int launch_select(naqs_ham_t *h, const A &a, hipStream_t s) {
    const int64_t n_ext = a.n;
    const int force = env_int("NAQS_SELECT_FORM", 0);       // tuning/testing: 0 auto, 1 one workgroup, 2 multi
    const bool one = force == 1 || (force != 2 && n_ext <= ONE_MAX_ROWS);
    char name[96];
    if (one) {
        NAQS_KLAUNCH(select_one_kernel<A>, dim3(1), dim3(ONE_BLOCK), 0, s, a);
        std::snprintf(name, sizeof(name), "select_one_kernel");
    } else {
        const int64_t n_wg = (n_ext + MULTI_TILE - 1) / MULTI_TILE;
        SelectScratch *sc = ham_select_scratch(h);
        if (n_wg > sc->tiles) {
            const int64_t cap = head_room(n_wg, 64);
            const int st = regrow(sc->words, sc->tiles, cap, ((size_t)HIST_WORDS + 3 * (size_t)cap) * sizeof(uint32_t));
            if (st != NAQS_OK) return st;
        }
        uint32_t *ghist = sc->words, *wg_cnt = ghist + HIST_WORDS, *wg_intr = wg_cnt + sc->tiles, *wg_off = wg_intr + sc->tiles;
        HIP_TRY(hipMemsetAsync(ghist, 0, HIST_WORDS * sizeof(uint32_t), s));
        for (int p = 0; p < DIGITS; ++p) NAQS_KLAUNCH(select_hist_kernel<A>, dim3((unsigned)n_wg), dim3(MULTI_BLOCK), 0, s, a, ghist, p);
        NAQS_KLAUNCH(select_count_kernel<A>, dim3((unsigned)n_wg), dim3(MULTI_BLOCK), 0, s, a, ghist, wg_cnt, wg_intr);
        NAQS_KLAUNCH(select_scan_kernel, dim3(1), dim3(ONE_BLOCK), 0, s, n_wg, wg_cnt, wg_intr, wg_off, a.count);
        NAQS_KLAUNCH(select_scatter_kernel<A>, dim3((unsigned)n_wg), dim3(MULTI_BLOCK), 0, s, a, ghist, wg_off);
        std::snprintf(name, sizeof(name), "select_hist_kernel x8 + select_count_kernel + select_scan_kernel + select_scatter_kernel");
    }
    HIP_TRY(hipGetLastError());
    ham_set_last_kernel(h, name);
    return NAQS_OK;
}

}  // namespace

NAQS_API int naqs_ham_pt2_select(naqs_ham_t *h, int64_t n_ext, const uint64_t *ext_keys_dev, const double *num_dev, const double *diag_dev,
                                 double e0, int64_t k, double eps_min, double tie_rtol, int64_t capacity, uint64_t *out_keys_dev,
                                 int64_t *count_dev, void *stream) {
    if (!h || n_ext < 0 || capacity < 0 || !count_dev || !std::isfinite(e0)) return NAQS_ERR_INVALID;
    if (!(eps_min >= 0) || !(tie_rtol >= 0)) return NAQS_ERR_INVALID;            // negative or NaN
    if (n_ext > 0 && (!ext_keys_dev || !num_dev || !diag_dev)) return NAQS_ERR_INVALID;
    if (capacity > 0 && !out_keys_dev) return NAQS_ERR_INVALID;
    if (n_ext > (1ll << 30)) return NAQS_ERR_UNSUPPORTED;                         // naqs_ham_connected's limit; counts are 32-bit words
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DeviceGuard guard;
    int st = guard.init(ham_device(h));
    if (st != NAQS_OK) return st;
    if (n_ext == 0) {
        HIP_TRY(hipMemsetAsync(count_dev, 0, 2 * sizeof(int64_t), s));
        return NAQS_OK;
    }
    SelArgs a{n_ext, ext_keys_dev, num_dev, diag_dev, e0, eps_min, 1.0 - tie_rtol, k, capacity, out_keys_dev, count_dev};
    return launch_select(h, a, s);
}

NAQS_API int naqs_ham_pt2_select_avg(naqs_ham_t *h, int64_t n_ext, const uint64_t *ext_keys_dev, int32_t nb, const double *num_dev,
                                     const double *diag_dev, const double *e_host, const double *w_host, int64_t k, double eps_min,
                                     double tie_rtol, int64_t capacity, uint64_t *out_keys_dev, int64_t *count_dev, void *stream) {
    if (!h || n_ext < 0 || capacity < 0 || !count_dev || !e_host || !w_host || nb < 1 || nb > MAX_ROOTS) return NAQS_ERR_INVALID;
    if (!(eps_min >= 0) || !(tie_rtol >= 0)) return NAQS_ERR_INVALID;            // negative or NaN
    SelAvgArgs a{};
    for (int j = 0; j < nb; ++j) {
        if (!(w_host[j] >= 0) || !std::isfinite(w_host[j])) return NAQS_ERR_INVALID;
        if (w_host[j] == 0) continue;                                             // not a live root: its row and energy are never read
        if (!std::isfinite(e_host[j])) return NAQS_ERR_INVALID;
        a.e[a.n_live] = e_host[j]; a.w[a.n_live] = w_host[j]; a.col[a.n_live] = j;
        ++a.n_live;
    }
    if (a.n_live == 0) return NAQS_ERR_INVALID;
    if (n_ext > 0 && (!ext_keys_dev || !num_dev || !diag_dev)) return NAQS_ERR_INVALID;
    if (capacity > 0 && !out_keys_dev) return NAQS_ERR_INVALID;
    if (n_ext > (1ll << 30)) return NAQS_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DeviceGuard guard;
    int st = guard.init(ham_device(h));
    if (st != NAQS_OK) return st;
    if (n_ext == 0) {
        HIP_TRY(hipMemsetAsync(count_dev, 0, 2 * sizeof(int64_t), s));
        return NAQS_OK;
    }
    a.n = n_ext; a.keys = ext_keys_dev; a.num = num_dev; a.diag = diag_dev;
    a.eps_min = eps_min; a.factor = 1.0 - tie_rtol; a.k = k; a.capacity = capacity; a.out = out_keys_dev; a.count = count_dev;
    return launch_select(h, a, s);
}
