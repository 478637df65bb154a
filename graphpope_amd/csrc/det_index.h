// The inverted index of deterministic mode (sage_set_deterministic), stated once for its two users: sage.hip (per source row, the
// destinations that list it) and node2vec.hip (per node, the entries that name it).  A counting sort in the caller's scratch buffer:
//
//     start [n + 1] | list [m] | sorted [m]        int32 each; n keys (sources / nodes), m slots (block slots / entries)
//
//   clear   start[0 .. n] = 0                                                    det_clear_body
//   count   start[j] = slots that name key j (integer atomics: no order in it)   the caller's producer, FILL = false
//   scan    start[j] = the FIRST slot of j's list (exclusive prefix sums)        det_scan_body
//   fill    every slot puts its value at list[start[j]++]                        the caller's producer, FILL = true
//
// After the fill start[j] is the END of j's list; the list begins at start[j - 1], or at 0 for j = 0 (det_list_bounds, which also
// clamps both to the slot count: a bad entry is skipped, never followed).  The CONTENT of a list does not depend on the order in which
// the fill's atomics arrive, the order inside it does: whoever sums a list orders it first, ascending.  A list of up to 64 values is
// sorted in registers (wave_sort_ascending); a longer one is ranked into `sorted`, value by value, by det_ranks_before.
//
// What differs stays with each caller, beside its __global__ wrappers: the producer of the slots, who ranks the long lists, the sum.
#pragma once

#include "wave.h"

namespace pope {

constexpr int DET_SCAN_THREADS = 1024, DET_SCAN_ITEMS = 8;        // one block; DET_SCAN_THREADS x DET_SCAN_ITEMS keys per round

// start[0 .. n] = 0; grid-stride, any grid.  (The kernel passes its own thread index and thread count: blockDim read inside a
// __device__ function compiles to the form for non-uniform groups, a dependent load in front of a kernel this short.)
__device__ __forceinline__ void det_clear_body(int *__restrict__ start, const long long n, const long long thread, const long long threads) {
    for (long long j = thread; j <= n; j += threads) start[j] = 0;
}

// start[0 .. n) -> its exclusive prefix sums, in place.  ONE block of DET_SCAN_THREADS threads; n < 2^31 (64-bit index arithmetic:
// base + DET_SCAN_THREADS x DET_SCAN_ITEMS may pass it).
__device__ __forceinline__ void det_scan_body(int *__restrict__ start, const long long n) {
    __shared__ int s_wave[DET_SCAN_THREADS / 64];
    __shared__ int s_carry;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (long long base = 0; base < n; base += DET_SCAN_THREADS * DET_SCAN_ITEMS) {
        const long long at = base + threadIdx.x * DET_SCAN_ITEMS;
        int v[DET_SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int k = 0; k < DET_SCAN_ITEMS; ++k) {
            v[k] = at + k < n ? start[at + k] : 0;
            sum += v[k];
        }
        const int incl = wave_inclusive_scan(sum, lane);            // the threads' sums inside the wave ...
        if (lane == 63) s_wave[wib] = incl;
        __syncthreads();
        int run = s_carry + incl - sum;                             // ... plus the waves in front and the rounds before
        for (int w = 0; w < wib; ++w) run += s_wave[w];
#pragma unroll
        for (int k = 0; k < DET_SCAN_ITEMS; ++k) {
            if (at + k < n) start[at + k] = run;
            run += v[k];
        }
        __syncthreads();
        if (threadIdx.x == DET_SCAN_THREADS - 1) s_carry = run;
        __syncthreads();
    }
}

// [beg, end) of key j's list after the fill, both clamped to [0, cap], cap = the slots the fill can have written.
__device__ __forceinline__ void det_list_bounds(const int *__restrict__ start, const long long j, const int cap, int &beg, int &end) {
    beg = min(max(j ? start[j - 1] : 0, 0), cap);
    end = min(max(start[j], beg), cap);
}

// Does the value `o` at list position pos_o come before `mine` at pos_mine in the ascending order?  Ties are broken by position, so
// the rank of a value (the number of values before it) is a permutation of the list even when it holds a value twice.
__device__ __forceinline__ bool det_ranks_before(const int o, const int mine, const long long pos_o, const long long pos_mine) {
    return o < mine || (o == mine && pos_o < pos_mine);
}

// What both sums over a list share (sage.hip: k_scatter_sum_det, aggregate.hip: k_scatter_ordered).  One 256-column slab of a source row:
// VEC lane l owns columns c0 + 4 l .. 4 l + 3 (one 16-byte access), otherwise c0 + l, l + 64, l + 128, l + 192.
template <bool VEC>
__device__ __forceinline__ void det_row_begin(const float *gx, const int j, const bool keep, const int C, const int c0, const int lane,
                                              float (&acc)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = 0.f;
    if (!keep) return;
    const float *row = gx + (size_t)j * C;
    if (VEC) {
        const int c = c0 + 4 * lane;
        if (c < C) {
            const float4 q = *reinterpret_cast<const float4 *>(row + c);
            acc[0] = q.x; acc[1] = q.y; acc[2] = q.z; acc[3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + k * 64 + lane;
            if (c < C) acc[k] = row[c];
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void det_row_end(float *gx, const int j, const int C, const int c0, const int lane, const float (&acc)[4]) {
    float *row = gx + (size_t)j * C;
    if (VEC) {
        const int c = c0 + 4 * lane;
        if (c < C) *reinterpret_cast<float4 *>(row + c) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + k * 64 + lane;
            if (c < C) row[c] = acc[k];
        }
    }
}

}  // namespace pope
