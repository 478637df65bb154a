// Full-wave (64 lanes) folds, scan, sort and broadcast, each written once.  Every one is a fixed pattern of lane exchanges: the result
// does not depend on scheduling, and where every lane returns the result, every lane returns the same bits.  The callers' bit-level
// contracts (fixed-order float64 sums, the row loss shared by training and evaluation, the ordered lists of deterministic mode) rest
// on that.  Partial-width folds (16 or 32 lanes of a tile layout) stay with their one caller.
#pragma once

#include <hip/hip_runtime.h>

namespace pope {

// Sum over the wave by the xor butterfly 32, 16, ... 1: at every step lane l adds lane (l ^ off)'s partial to its own.  T: float,
// double, int, unsigned, unsigned long long.  Floating-point: the order is fixed and addition commutes, so all lanes end with the same bits.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// Maximum over the wave, the same butterfly (fmaxf: a NaN lane is dropped unless every lane holds one).
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// Inclusive prefix sum over the lanes: lane l returns v of lanes 0 .. l.
__device__ __forceinline__ int wave_inclusive_scan(int v, const int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// Ascending bitonic sort of one value per lane.
__device__ __forceinline__ int wave_sort_ascending(int v, const int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int o = __shfl_xor(v, j, 64);
            v = (((lane & j) == 0) == ((lane & k) == 0)) ? min(v, o) : max(v, o);
        }
    }
    return v;
}

// v of lane `src` in every lane; `src` is the same for the whole wave: two scalar reads.
__device__ __forceinline__ double wave_read_lane(double v, int src) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

}  // namespace pope
