// What both tile kernels of the node2vec-space embedding (pairwise.hip: k_pairwise, pairwise_persistent.h:
// k_pairwise_persistent) share: the row-norm pair, the wave-wide squared distance and the metric epilogue of one 32 x 32
// accumulator.  What stays in each kernel is what differs: where the norms come from, how anchor rows are addressed, the
// stores and the min / max bookkeeping.
#pragma once

#include "gemm_tile.h"   // f32x16, common.h
#include "wave.h"

namespace pope {

typedef float f32x4v __attribute__((ext_vector_type(4)));

// Euclidean cancellation threshold: an output with d2 < PW_CANCEL_RATIO * (|x|^2 + |a|^2) is recomputed as a direct sum of
// squared differences.  The f32 expansion's error on the scaled value grows as the ratio falls (rows that share an offset,
// and with the depth): measured over tests/pairwise_cases.py on every kernel path, the largest error among the outputs at a
// ratio >= 2^-7 was 5.7e-5, >= 2^-5 1.6e-5, >= 2^-4 7.6e-6, >= 2^-3 3.6e-6.  2^-3 is the smallest power of two that stays
// within HALF the 1e-5 gate (the cases are a finite sample of seeds); it was 1e-2 before.  It costs nothing
// on a zero-mean table: the smallest ratio among the benchmark's 2.3e7 pairs (N(0, 1), D = 128) is 0.547.
// tests/pairwise_cases.py states the same value (CANCEL_RATIO) and derives its cases from it.
constexpr float PW_CANCEL_RATIO = 0.125f;

// What the epilogue takes from a row's f64 sum of squares: {(float)|r|^2, 1 / |r|}, with the factor 1 for a row whose
// squared norm is 0 IN FLOAT32 -- a zero row, and a row whose squares underflow (components ~1e-25: the f64 sum is not 0,
// 1 / sqrtf((float)sum) would be inf and a cosine output 0 * inf = NaN).  sklearn normalize() in float32 leaves both as they are.
__device__ __forceinline__ float2 row_norm_pair(double sumsq) {
    const float s = (float)sumsq;
    return make_float2(s, s == 0.0f ? 1.0f : 1.0f / sqrtf(s));
}

// sum_k (x[k] - a[k])^2 by a whole wave: lane l takes k = l, l + 64, ...; fixed shuffle tree, so the value does not
// depend on scheduling.  Every lane returns the total.
__device__ __forceinline__ float wave_sqdist(const float *__restrict__ x, const float *__restrict__ a, int D, int lane) {
    float acc = 0.0f;
    for (int k = lane; k < D; k += 64) {
        const float d = x[k] - a[k];
        acc = fmaf(d, d, acc);
    }
    return wave_sum(acc);
}

// The metric epilogue of one 32 x 32 accumulator (C/D layout: col = lane & 31, register r holds row row_base + (r & 3) +
// 8 * (r >> 2), row_base = the tile's first row + 4 * (lane >> 5)): e[r] = the raw metric value of output r.
//   xr[r]     what the metric uses of that row: (float)|x|^2 (euclidean) or 1 / |x| (cosine)
//   a2f, rna  the column's (float)|a|^2 and 1 / |a|
//   FULL      all 32 rows and this lane's column exist: no per-output predicate; else output r is live if its row < N && col_ok
//   anchor_at(col) -> the anchor row of column col in global memory, for the recomputation
// It is instruction-bound (16 outputs per lane), so everything that depends on the row only is the caller's to hoist and the
// per-element arithmetic is f32: the f32-accumulated MFMA dot carries ~1e-6 of |x||a| already, a f64 sum of the norms on top
// of it buys nothing (the reference's f64 accuracy is restored where it matters, by the fix-up below).
template <bool FULL, class AnchorAt>
__device__ __forceinline__ void pw_metric_epilogue(float (&e)[16], const f32x16 &acc, const float (&xr)[16], float a2f, float rna, int metric,
                                                   int row_base, int N, bool col_ok, int col, const float *__restrict__ X, int D, int lane,
                                                   AnchorAt anchor_at) {
    if (metric == POPE_METRIC_EUCLIDEAN) {
        float margin = __builtin_huge_valf();                 // min over the live outputs of d2 - PW_CANCEL_RATIO (|x|^2 + |a|^2): negative = digits lost
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float norms = xr[r] + a2f;
            e[r] = fmaf(-2.0f, acc[r], norms);                // squared distance
            const bool live = FULL || (row_base + (r & 3) + 8 * (r >> 2) < N && col_ok);
            if (live) margin = fminf(margin, fmaf(-PW_CANCEL_RATIO, norms, e[r]));
        }
        // cancellation (an anchor against its own row, coincident rows, rows that share an offset): recompute exactly as a sum
        // of squared differences.  Rare on a zero-mean table, and kept out of the straight-line code above: ONE wave-wide test
        // per tile, then the whole wave does each flagged output together -- 64 lanes over the depth, shuffle reduction --
        // instead of one lane walking D dependent loads while the other 63 wait (that was a 90 us tail on a 140 us kernel).
        if (__any(margin < 0.0f)) {
            for (int r = 0; r < 16; ++r) {
                const int row = row_base + (r & 3) + 8 * (r >> 2);
                float er = 0.0f, nr = 0.0f;
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (q == r) { er = e[q]; nr = xr[q] + a2f; }
                unsigned long long fix = __ballot((FULL || (row < N && col_ok)) && er < PW_CANCEL_RATIO * nr);
                while (fix) {
                    const int src = __ffsll((long long)fix) - 1;
                    fix &= fix - 1;
                    const int acol = __shfl(col, src);
                    const float v = wave_sqdist(X + (size_t)__shfl(row, src) * D, anchor_at(acol), D, lane);
                    if (lane == src) {
#pragma unroll
                        for (int q = 0; q < 16; ++q)
                            if (q == r) e[q] = v;
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) e[r] = __builtin_amdgcn_sqrtf(fmaxf(e[r], 0.0f));   // v_sqrt_f32 (1 ulp): the IEEE expansion is ~15 instructions per output
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float sim = acc[r] * xr[r] * rna;
            e[r] = metric == POPE_METRIC_COSINE_SIMILARITY ? sim : fminf(fmaxf(1.0f - sim, 0.0f), 2.0f);
        }
    }
}

}  // namespace pope
