// naqs_common.hpp — host-side helpers shared by the translation units of libnaqs_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>

#include "naqs_hip.h"

#define NAQS_API extern "C" __attribute__((visibility("default")))

namespace naqs {

extern thread_local hipError_t g_last_hip;   // defined in naqs_hip.hip

#define HIP_TRY(expr)                                  \
    do {                                               \
        hipError_t e__ = (expr);                       \
        if (e__ != hipSuccess) {                       \
            ::naqs::g_last_hip = e__;                  \
            return NAQS_ERR_HIP;                       \
        }                                              \
    } while (0)

constexpr int WAVE = 64;

// every kernel launch of the library goes through this (naqs_launch_count(): bench.py's launches per training step)
extern std::atomic<int64_t> g_launches;      // defined in naqs_hip.hip
#define NAQS_KLAUNCH(...)                                                  \
    do {                                                                   \
        ::naqs::g_launches.fetch_add(1, std::memory_order_relaxed);        \
        hipLaunchKernelGGL(__VA_ARGS__);                                   \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    int init(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) return NAQS_ERR_NO_DEVICE;
        if (prev != dev) {
            HIP_TRY(hipSetDevice(dev));
            switched = true;
        }
        return NAQS_OK;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

inline int env_int(const char *name, int dflt) {
    const char *v = std::getenv(name);
    return v ? std::atoi(v) : dflt;
}

// A handle's scratch array that grows on demand and never shrinks: wait for the device (a launch in flight, on any stream, may
// still read the old array), free it, allocate `bytes` for `new_cap` entries, record the capacity (0 while there is no array).
// head_room: the capacity asked for n entries, a quarter more, so that a slowly growing n does not come back every call.
inline int64_t head_room(int64_t n, int64_t least) { return n + n / 4 > least ? n + n / 4 : least; }
template <typename T>
inline int regrow(T *&ptr, int64_t &cap, int64_t new_cap, size_t bytes) {
    HIP_TRY(hipDeviceSynchronize());
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr; cap = 0;
    HIP_TRY(hipMalloc((void **)&ptr, bytes));
    cap = new_cap;
    return NAQS_OK;
}

// HIP-event pairs around the launches of one kernel (bench.py's roofline leg)
struct EventRing {
    hipEvent_t *ev = nullptr;
    int cap = 0, used = 0;
    int stride = 1, tick = 0;            // record every stride-th launch (an event pair costs ~4 us of queue time)
    int enable(int max_records) {
        for (int i = 0; i < cap; ++i) (void)hipEventDestroy(ev[i]);
        std::free(ev);
        ev = nullptr; cap = used = 0; tick = 0;
        if (max_records <= 0) return NAQS_OK;
        ev = static_cast<hipEvent_t *>(std::calloc((size_t)2 * max_records, sizeof(hipEvent_t)));
        if (!ev) return NAQS_ERR_NOMEM;
        for (int i = 0; i < 2 * max_records; ++i) { HIP_TRY(hipEventCreate(&ev[i])); cap = i + 1; }
        return NAQS_OK;
    }
    bool armed() { return used + 2 <= cap && (tick++ % stride) == 0; }
    int begin(hipStream_t s) { HIP_TRY(hipEventRecord(ev[used], s)); return NAQS_OK; }
    int end(hipStream_t s) { HIP_TRY(hipEventRecord(ev[used + 1], s)); used += 2; return NAQS_OK; }
    int read(double *total_ms, int64_t *launches) {
        double tot = 0;
        for (int i = 0; i + 1 < used; i += 2) {
            HIP_TRY(hipEventSynchronize(ev[i + 1]));
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            tot += ms;
        }
        *total_ms = tot;
        *launches = used / 2;
        used = 0;
        return NAQS_OK;
    }
};

struct ElocFeed;
// implemented in naqs_hip.hip; used by the fused entry point naqs_logpsi_eloc
int eloc_begin(naqs_ham *h, int64_t M, hipStream_t s, ElocFeed *feed);
int eloc_main(naqs_ham *h, int64_t M, const ElocFeed &feed, double *eloc_dev, const double *w_dev, double *out4_dev,
              hipStream_t s);
int ham_device(const naqs_ham *h);
// naqs_ham_pt2_select (naqs_select.hip): the handle owns its scratch (histograms and per-tile words of the multi-workgroup form,
// grown there on demand, freed by naqs_ham_destroy) and reports its form through naqs_ham_last_kernel
struct SelectScratch {
    uint32_t *words = nullptr;
    int64_t tiles = 0;
};
SelectScratch *ham_select_scratch(naqs_ham *h);
void ham_set_last_kernel(naqs_ham *h, const char *name);
// naqs_ham_eig_lowest (naqs_eig.hip): the handle owns the solver's scratch (basis, diagonal, correction, per-tile partial sums and
// the small problem, one array grown there on demand, freed by naqs_ham_destroy).  ham_eig_begin builds the key table of one
// solve; ham_eig_product launches the row walk of naqs_ham_pt2 on it, the rows being the table's own keys:
// num_i = sum_{j != i} H_ij v_j and diag_i = H_ii, so H v = num + diag * v.
// ham_eig_block_product (naqs_ham_block_product, naqs_ham_eig_lowest_k) is that product for nb <= 8 vectors on one walk: vector
// c is src[slots[c] * ld + i], num[c * ldn + i] its product; the vectors are first laid out [M][4 or 8] in `pack`.
struct EigScratch {
    double *buf = nullptr;
    int64_t doubles = 0;
    double *pack = nullptr;
    int64_t pack_doubles = 0;
};
EigScratch *ham_eig_scratch(naqs_ham *h);
const char *ham_last_kernel_name(const naqs_ham *h);
int ham_eig_begin(naqs_ham *h, int64_t M, const uint64_t *keys_dev, hipStream_t s, ElocFeed *feed);
int ham_eig_product(naqs_ham *h, int64_t M, const uint64_t *keys_dev, const ElocFeed &feed, const double *v_dev, double *num_dev,
                    double *diag_dev, hipStream_t s);
int ham_eig_block_product(naqs_ham *h, int64_t M, const uint64_t *keys_dev, const ElocFeed &feed, int nb, const double *src_dev,
                          int64_t ld, const int32_t *slots, double *num_dev, int64_t ldn, double *diag_dev, hipStream_t s);
int net_device(const naqs_net *n);           // implemented in naqs_logpsi.hip

}  // namespace naqs
