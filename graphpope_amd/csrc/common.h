// Shared host-side helpers for libgraphpope_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "graphpope_hip.h"

namespace pope {

typedef unsigned long long u64;

// Per-thread error string behind pope_last_error().
void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void clear_error();

inline int hip_fail(hipError_t e, const char *what, const char *file, int line) {
    set_error("%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    return POPE_ERR_HIP;
}

#define POPE_HIP(call)                                                         \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) return ::pope::hip_fail(e_, #call, __FILE__, __LINE__); \
    } while (0)

#define POPE_REQUIRE(cond, ...)                 \
    do {                                        \
        if (!(cond)) {                          \
            ::pope::set_error(__VA_ARGS__);     \
            return POPE_ERR_INVALID;            \
        }                                       \
    } while (0)

// Diagnostic knobs behind pope_debug_set() (abi.cpp; include/graphpope_hip.h documents the values): process-global, not thread-safe,
// A/B tooling and tests only.  Every module owns its own.
struct FinalizeKnobs {                 // the finalise kernels (geodesic.hip: finalize_plan)
    int variant = 1;                   // 1: pipelined / wide fast paths (default), 7: round 1-3 fast path, 0: generic kernel -- kept so the tests can compare their bits
    int blocks = 256 * 8;              // POPE_KNOB_FINALIZE_BLOCKS: the round 1-3 kernel's grid ...
    bool blocks_set = false;           // ... and, once given, the pipelined kernels' too (default: one work item per wave)
    int shard_batches = 1;             // k_finalize_lut over several short-rowed shards: 1 = a batch per (shard, block of rows), 0 = the flat order (variant 11 / 12)
    int lut = 1;                       // wide rows: 1 (default) k_finalize_lut for rows without features, k_finalize_wide with them (copy kernel + table kernel measured slower: Flickr / 1 024 anchors 0.619 against 0.562 ms); 2 always; 0 never (variant 8 / 9 / 10)
};
struct GeodesicKnobs {                 // defined in geodesic.hip
    int live_mode = -1;                // -1: by graph size (LDS table up to LIVE_MAX_NODES, global table beyond); 2 / 3: the global table on a small graph too (tests)
    FinalizeKnobs fin;
    int prepare_merge = 1;             // 1 (default) = pope_geodesic_run clears, seeds and builds the CSR in ONE launch (k_prepare); 0 = two launches
    int level1_apply = 1;              // 1 (default) = behind k_prepare, level 1 comes from the hit lists its CSR role records (k_bfs_level1_apply); 0 = a level launch
    int level_compact = 16;            // POPE_KNOB_LEVEL_COMPACT: chunks of the LDS-table level kernels with at most this many live slots (up to 64) take the compacted path (geodesic_level.h); 0 = none does
};
extern GeodesicKnobs g_geodesic;
extern int g_sage_forward_overlap, g_forward_whole_tiles, g_gemm_tile16_buffers, g_streamk_xcd;   // sage.hip
extern int g_sage_deterministic;       // sage.hip: sage_set_deterministic (not a diagnostic knob: a mode of the library)
extern int g_pairwise_kernel;          // pairwise.hip
extern int g_copy_batches_per_wave;    // side_copy.hip
extern int g_fail_host_register;       // abi.cpp, for host.cc

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// "The LDS opt-in of these kernels has been applied on the current device": one bit per device, set AFTER the attribute
// calls have returned, so neither a second device nor a second host thread can launch a >64 KB-LDS kernel without it
// (two threads may both apply it: hipFuncSetAttribute is idempotent).  Usage:
//     static LdsOptIn once;  if (!once.done()) { POPE_HIP(hipFuncSetAttribute(...)); ...; once.mark(); }
struct LdsOptIn {
    std::atomic<unsigned long long> mask[2] = {{0}, {0}};          // devices 0 .. 127
    static int device() {
        int dev = 0;
        return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 128 ? dev : -1;
    }
    bool done() const {
        const int d = device();
        return d >= 0 && ((mask[d >> 6].load(std::memory_order_acquire) >> (d & 63)) & 1ull);
    }
    void mark() {
        const int d = device();
        if (d >= 0) mask[d >> 6].fetch_or(1ull << (d & 63), std::memory_order_release);
    }
};

// Words of 64 anchors per node, padded so a node's words form whole tiles of 1, 2 or 4 words.
inline int words_for(int K) {
    int w = (K + 63) / 64;
    if (w <= 2) return w < 1 ? 1 : w;
    return (w + 3) / 4 * 4;
}

// Device extents (include/graphpope_hip.h, "dims"): a size that is only known on the device.  `cap` is the host-side capacity
// the launch was sized for; a null pointer means the capacity IS the size.
__device__ __forceinline__ int dyn_extent(const int *dev, int cap) {
    if (!dev) return cap;
    const int v = *dev;
    return v < cap ? (v < 0 ? 0 : v) : cap;
}

// Compute units of the current device, looked up once per device.
inline int device_cu_count(int *out) {
    static int cus[64];
    int dev = 0;
    POPE_HIP(hipGetDevice(&dev));
    POPE_REQUIRE(dev >= 0 && dev < 64, "device index %d out of range", dev);
    if (!cus[dev]) POPE_HIP(hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev));
    *out = cus[dev];
    return POPE_OK;
}

// Memory-bound grids: enough blocks to fill 256 CUs several times over, grid-stride the rest.
inline unsigned capped_grid(size_t work_items, unsigned block, unsigned cap = 256u * 16u) {
    size_t b = (work_items + block - 1) / block;
    if (b < 1) b = 1;
    return (unsigned)(b > cap ? cap : b);
}

}  // namespace pope
