// SAGEConv(aggr='add' | 'max') on MI355X (gfx950): the aggregation half of the layer for the two other aggregators PyG 1.7.0's SAGEConv
// takes (matmul(adj_t, x, reduce='add' | 'max')), forward and backward.  The projections stay where they are (sage.hip): a precomputed
// agg goes to the same GEMM calls as the mean's.  include/graphpope_hip.h, "Sum and max aggregation", is the contract both kernels keep
// bit for bit.
//
//   k_gather_reduce<OP, VEC>    agg[i] = sum or max over row i's slots of x[col[p]], ONE accumulator per column, slots ascending; max also
//                               records the winning block-local source (arg).  k_gather_mean's structure: one wave per destination row,
//                               16-byte lane accesses along the feature dimension (VEC), four neighbour rows requested before the first is
//                               folded, n_id / x_dst of indexed mode, device extents.  No LDS, no scratch.
//   k_scatter_ordered<OP, VEC>  grad_x[j] = (j < n_dst ? grad_x[j] : +0) + the terms of j's slots in ascending slot order, over the inverted
//                               index of det_index.h (built by sage.hip's k_det_* launches): one wave per (source row, 256-column slab),
//                               k_scatter_sum_det's structure.  No float atomics in either mode of the library; add lets a destination
//                               that lists j twice contribute twice, max once and only in the columns whose recorded arg is j.
// Neither kernel multiplies, so there is nothing for -ffp-contract to fuse: the sums are the plain additions the contract writes.
// Every index read from the block (rowptr, col, n_id, the lists) is range-checked and every loop is bounded by a row or list length.
#include "aggregate.h"
#include "det_index.h"

namespace pope {

// The row of x that block-local source j lives in, or -1 for a j or an n_id entry out of range (the slot is then skipped).
__device__ __forceinline__ long long reduce_src_row(const int j, const int n_src, const long long *__restrict__ n_id, const long long x_rows) {
    if ((unsigned)j >= (unsigned)n_src) return -1;
    const long long r = n_id ? n_id[j] : (long long)j;
    return (unsigned long long)r < (unsigned long long)x_rows ? r : -1;
}

// W columns of row r at piece q (VEC: one 16-byte access); zeros, unread, for a skipped slot.
template <bool VEC>
__device__ __forceinline__ void reduce_load(const float *__restrict__ x, const long long r, const int C, const int q, float (&v)[VEC ? 4 : 1]) {
    if constexpr (VEC) {
        const float4 t = r >= 0 ? reinterpret_cast<const float4 *>(x + (size_t)r * C)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = r >= 0 ? x[(size_t)r * C + q] : 0.f;
    }
}

// One slot folded into the accumulators.  add: s + v.  max: v replaces s (and j the recorded source) iff v > s, or v is NaN and s is
// not -- so ties stay with the first slot and the first NaN stays to the end; the first slot of a row is taken as it is (`have`).
template <int OP, int W>
__device__ __forceinline__ void reduce_fold(float (&s)[W], int (&a)[W], bool &have, const float (&v)[W], const int j) {
    if (OP == POPE_AGGR_ADD) {
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] = s[k] + v[k];
        return;
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const bool take = !have || v[k] > s[k] || (v[k] != v[k] && s[k] == s[k]);
        if (take) { s[k] = v[k]; a[k] = j; }
    }
    have = true;
}

template <int OP, bool VEC>
__global__ __launch_bounds__(256) void k_gather_reduce(const int *__restrict__ rowptr, const int *__restrict__ col, int n_dst, int n_src, const int nnz,
                                                       const float *__restrict__ x, const long long x_rows, const int C, float *__restrict__ agg,
                                                       int *__restrict__ arg, const long long *__restrict__ n_id, float *__restrict__ x_dst,
                                                       const int *__restrict__ dims) {
    constexpr int W = VEC ? 4 : 1;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    n_dst = dyn_extent(dims, n_dst);
    n_src = dyn_extent(dims ? dims + 1 : nullptr, n_src);
    const int pieces = VEC ? C >> 2 : C;                               // per row: 16-byte pieces, or single columns
    for (int i = wave; i < n_dst; i += nwaves) {
        const int beg = min(max(rowptr[i], 0), nnz), end = min(max(rowptr[i + 1], beg), nnz);
        const long long own = x_dst ? reduce_src_row(i, n_src, n_id, x_rows) : -1;
        for (int q = lane; q < pieces; q += 64) {
            float s[W];
            int a[W];
#pragma unroll
            for (int k = 0; k < W; ++k) { s[k] = 0.f; a[k] = -1; }
            bool have = false;
            int p = beg;
            for (; p + 3 < end; p += 4) {                              // four neighbour rows in flight
                int j[4];
                long long r[4];
                float v[4][W];
#pragma unroll
                for (int u = 0; u < 4; ++u) j[u] = col[p + u];
#pragma unroll
                for (int u = 0; u < 4; ++u) r[u] = reduce_src_row(j[u], n_src, n_id, x_rows);
#pragma unroll
                for (int u = 0; u < 4; ++u) reduce_load<VEC>(x, r[u], C, q, v[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (r[u] >= 0) reduce_fold<OP, W>(s, a, have, v[u], j[u]);
            }
            for (; p < end; ++p) {
                const int j = col[p];
                const long long r = reduce_src_row(j, n_src, n_id, x_rows);
                float v[W];
                reduce_load<VEC>(x, r, C, q, v);
                if (r >= 0) reduce_fold<OP, W>(s, a, have, v, j);
            }
            if constexpr (VEC) {
                reinterpret_cast<float4 *>(agg + (size_t)i * C)[q] = make_float4(s[0], s[1], s[2], s[3]);
                if (OP == POPE_AGGR_MAX && arg) reinterpret_cast<int4 *>(arg + (size_t)i * C)[q] = make_int4(a[0], a[1], a[2], a[3]);
                if (own >= 0) reinterpret_cast<float4 *>(x_dst + (size_t)i * C)[q] = reinterpret_cast<const float4 *>(x + (size_t)own * C)[q];
            } else {
                agg[(size_t)i * C + q] = s[0];
                if (OP == POPE_AGGR_MAX && arg) arg[(size_t)i * C + q] = a[0];
                if (own >= 0) x_dst[(size_t)i * C + q] = x[(size_t)own * C + q];
            }
        }
    }
}

// acc += the terms of the `cnt` list entries the lanes hold (lane t: destination `ids`, counted iff `use`), strictly in lane order.
// add: the term is grad_agg[i]; max: grad_agg[i] in the columns whose arg[i] is j, nothing in the others -- nothing, not +0: a -0 found in
// grad_x stays -0.  AHEAD rows are requested before the first addition of a round; past the end the last row again, loaded and not added.
template <int OP, bool VEC>
__device__ __forceinline__ void ordered_add_rows(const int ids, const bool use, const int cnt, const int j, const float *__restrict__ gagg,
                                                 const int *__restrict__ arg, const int C, const int c0, const int lane, float (&acc)[4]) {
    constexpr int AHEAD = OP == POPE_AGGR_MAX ? 4 : 8;                 // (max holds the arg row beside every gradient row)
    for (int t0 = 0; t0 < cnt; t0 += AHEAD) {
        float r[AHEAD][4];
        int ar[AHEAD][4];
        bool on[AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int t = min(t0 + u, cnt - 1);
            const size_t at = (size_t)__shfl(ids, t) * C;
            on[u] = __shfl((int)use, t) != 0 && t0 + u < cnt;
            if (VEC) {
                const int c = c0 + 4 * lane;
                const float4 g = c < C ? *reinterpret_cast<const float4 *>(gagg + at + c) : make_float4(0.f, 0.f, 0.f, 0.f);
                r[u][0] = g.x; r[u][1] = g.y; r[u][2] = g.z; r[u][3] = g.w;
                if (OP == POPE_AGGR_MAX) {
                    const int4 w = c < C ? *reinterpret_cast<const int4 *>(arg + at + c) : make_int4(-1, -1, -1, -1);
                    ar[u][0] = w.x; ar[u][1] = w.y; ar[u][2] = w.z; ar[u][3] = w.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = c0 + k * 64 + lane;
                    r[u][k] = c < C ? gagg[at + c] : 0.f;
                    if (OP == POPE_AGGR_MAX) ar[u][k] = c < C ? arg[at + c] : -1;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            if (!on[u]) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (OP == POPE_AGGR_ADD || ar[u][k] == j) acc[k] = acc[k] + r[u][k];
        }
    }
}

// One wave per (source row j, 256-column slab).  A list of up to 64 destinations is sorted in registers; a longer one is ranked entry by
// entry into `sorted` by the wave of slab 0, which then sums every slab of the row (k_scatter_sum_det's two cases).  Ordering by destination
// is ordering by slot, and a destination that names j twice stands twice in the list, side by side once sorted: add counts both, max
// skips an entry equal to its predecessor.  A list entry outside [0, n_dst) is skipped, never followed.
template <int OP, bool VEC>
__global__ __launch_bounds__(256) void k_scatter_ordered(const int *__restrict__ start, const int *__restrict__ list, int *sorted, int n_dst, int n_src,
                                                         const int nnz, const int *__restrict__ arg, const float *__restrict__ gagg, const int C,
                                                         float *gx, const int *__restrict__ dims) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int slabs = (C + 255) / 256;
    n_dst = dyn_extent(dims, n_dst);
    n_src = dyn_extent(dims ? dims + 1 : nullptr, n_src);
    const long long items = (long long)n_src * slabs;
    for (long long w = wave; w < items; w += nwaves) {
        const int j = (int)(w / slabs), slab = (int)(w - (long long)j * slabs);
        int beg, end;
        det_list_bounds(start, j, nnz, beg, end);
        const int len = end - beg;
        const bool keep = j < n_dst;                                // the twin GEMM's row; the rows behind them start from +0
        if (len == 0 && keep) continue;
        float acc[4];
        if (len <= 64) {
            int ids = lane < len ? list[beg + lane] : 0x7fffffff;
            ids = wave_sort_ascending(ids, lane);
            const int before = __shfl_up(ids, 1, 64);
            bool use = (unsigned)ids < (unsigned)n_dst;
            if (OP == POPE_AGGR_MAX && lane > 0 && ids == before) use = false;
            if ((unsigned)ids >= (unsigned)n_dst) ids = 0;          // (the lanes past the list, or a bad entry: read in bounds, not counted)
            det_row_begin<VEC>(gx, j, keep, C, slab * 256, lane, acc);
            ordered_add_rows<OP, VEC>(ids, use, len, j, gagg, arg, C, slab * 256, lane, acc);
            det_row_end<VEC>(gx, j, C, slab * 256, lane, acc);
            continue;
        }
        if (slab != 0) continue;
        for (int e0 = 0; e0 < len; e0 += 64) {                      // rank of entry e = entries below it, ties broken by position
            const int e = e0 + lane;
            const int mine = e < len ? list[beg + e] : 0x7fffffff;
            int rank = 0;
            for (int m0 = 0; m0 < len; m0 += 64) {
                const int theirs = m0 + lane < len ? list[beg + m0 + lane] : 0x7fffffff;
                const int cnt = min(64, len - m0);
                for (int t = 0; t < cnt; ++t) {
                    const int o = __shfl(theirs, t);
                    rank += det_ranks_before(o, mine, m0 + t, e) ? 1 : 0;
                }
            }
            if (e < len) sorted[beg + rank] = mine;                 // (rank < len: a permutation of the list's positions)
        }
        __threadfence();                                            // the wave reads back what its other lanes wrote
        for (int s = 0; s < slabs; ++s) {
            det_row_begin<VEC>(gx, j, keep, C, s * 256, lane, acc);
            for (int p0 = 0; p0 < len; p0 += 64) {
                const int cnt = min(64, len - p0);
                int ids = lane < cnt ? sorted[beg + p0 + lane] : 0x7fffffff;
                const int before = lane < cnt && p0 + lane > 0 ? sorted[beg + p0 + lane - 1] : -1;
                bool use = (unsigned)ids < (unsigned)n_dst;
                if (OP == POPE_AGGR_MAX && ids == before) use = false;
                if ((unsigned)ids >= (unsigned)n_dst) ids = 0;
                ordered_add_rows<OP, VEC>(ids, use, cnt, j, gagg, arg, C, s * 256, lane, acc);
            }
            det_row_end<VEC>(gx, j, C, s * 256, lane, acc);
        }
    }
}

void enqueue_gather_reduce(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst, int64_t nnz, const float *x,
                           int64_t x_rows, int32_t c, int aggr, float *agg, int32_t *arg, float *x_dst, bool vec, const int32_t *dims,
                           hipStream_t stream) {
    const dim3 grid(capped_grid((size_t)n_dst * 64, 256));
    const long long *ids = (const long long *)n_id;
#define POPE_GATHER_REDUCE(OP, VEC)                                                                                                            \
    hipLaunchKernelGGL((k_gather_reduce<OP, VEC>), grid, dim3(256), 0, stream, rowptr, col, (int)n_dst, (int)n_src, (int)nnz, x, (long long)x_rows, c, \
                       agg, arg, ids, x_dst, dims)
    if (aggr == POPE_AGGR_ADD) {
        if (vec) POPE_GATHER_REDUCE(POPE_AGGR_ADD, true);
        else POPE_GATHER_REDUCE(POPE_AGGR_ADD, false);
    } else {
        if (vec) POPE_GATHER_REDUCE(POPE_AGGR_MAX, true);
        else POPE_GATHER_REDUCE(POPE_AGGR_MAX, false);
    }
#undef POPE_GATHER_REDUCE
}

void enqueue_scatter_ordered(const int32_t *rowptr, int64_t n_src, int64_t n_dst, int64_t nnz, const int *start, const int *list, int *sorted,
                             const int32_t *arg, const float *grad_agg, int32_t c, int aggr, float *grad_x, bool vec, const int32_t *dims,
                             hipStream_t stream) {
    (void)rowptr;                                                   // (no degree enters the sum: the index alone says who adds to whom)
    const dim3 grid(capped_grid((size_t)n_src * ((c + 255) / 256) * 64, 256));
#define POPE_SCATTER_ORDERED(OP, VEC)                                                                                                          \
    hipLaunchKernelGGL((k_scatter_ordered<OP, VEC>), grid, dim3(256), 0, stream, start, list, sorted, (int)n_dst, (int)n_src, (int)nnz, arg, grad_agg, \
                       c, grad_x, dims)
    if (aggr == POPE_AGGR_ADD) {
        if (vec) POPE_SCATTER_ORDERED(POPE_AGGR_ADD, true);
        else POPE_SCATTER_ORDERED(POPE_AGGR_ADD, false);
    } else {
        if (vec) POPE_SCATTER_ORDERED(POPE_AGGR_MAX, true);
        else POPE_SCATTER_ORDERED(POPE_AGGR_MAX, false);
    }
#undef POPE_SCATTER_ORDERED
}

}  // namespace pope

using namespace pope;

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The forward half on its own (include/graphpope_hip.h).
extern "C" int sage_aggregate_forward(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst, int64_t nnz,
                                      const float *x, int64_t x_rows, int32_t c, int32_t aggr, float *agg, int32_t *arg, float *x_dst,
                                      const int32_t *dims, void *stream_) {
    clear_error();
    POPE_REQUIRE(aggr == POPE_AGGR_ADD || aggr == POPE_AGGR_MAX, "sage_aggregate_forward: aggr %d is neither POPE_AGGR_ADD nor POPE_AGGR_MAX (the mean: sage_gather_mean)", aggr);
    POPE_REQUIRE(rowptr && (col || nnz == 0) && x && agg, "sage_aggregate_forward: null pointer");
    POPE_REQUIRE(!x_dst || n_id, "sage_aggregate_forward: x_dst is written in indexed mode only (n_id)");
    POPE_REQUIRE(n_dst > 0 && n_dst <= n_src && n_src < INT32_MAX && nnz >= 0 && nnz < INT32_MAX && c > 0 && x_rows > 0 && (n_id || x_rows >= n_src),
                 "sage_aggregate_forward: bad size (destinations must be the first n_dst sources; x holds every source)");
    const bool vec = (c & 3) == 0 && aligned16(x) && aligned16(agg) && aligned16(arg) && aligned16(x_dst);
    enqueue_gather_reduce(rowptr, col, n_id, n_src, n_dst, nnz, x, x_rows, c, aggr, agg, aggr == POPE_AGGR_MAX ? arg : nullptr, x_dst, vec, dims,
                          (hipStream_t)stream_);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}
