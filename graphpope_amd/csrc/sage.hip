// SAGEConv forward / backward on MI355X (gfx950) for the sampled bipartite blocks GraphPOPE trains on.
//
// Replaces the PyG SAGEConv call at /root/reference/main.py:206  x = convs[i]((x, x[:n_dst]), adj_t):
//     out = lin_l(mean_{j in N(i)} x_src[j]) + lin_r(x_src[i])          lin_l: weight + bias, lin_r: weight only
// (torch_sparse matmul(adj_t, x, reduce='mean') + two torch Linear layers in the reference stack).
//
//   k_gather_mean    neighbour gather + mean over the CSR block: one wave per destination row, 16-byte lane
//                    accesses along the feature dimension, several neighbour rows in flight.  HBM / L2 bound.
//   k_gemm           exact-f32 MFMA (v_mfma_f32_32x32x2_f32) tile, 128 x 256 or 64 x 128 per block, operands staged through
//                    LDS; C = sum_p A_p * B_p (+ bias) with p <= 2, so lin_l(agg) + lin_r(x_dst) is ONE pass
//                    that never materialises either product.  Arbitrary strides cover NT / NN / TN shapes;
//                    split-K (grid.z) with partial slabs + k_slab_reduce for the weight gradients
//                    (reduction over ~40 000 rows), deterministic: no float atomics there.
//   k_gemm_streamk_ld / k_gemm_streamk_tn   (gemm_streamk.h, gemm_streamk_tn.h) the two big products of a layer -- the forward
//                    projection and the weight-gradient twin -- as stream-K over one persistent block per CU: LDS-DMA staging by
//                    loader waves, MFMA-only consumer waves, partial tiles to slabs + a fix-up launch that sums them in block
//                    order; shapes they do not take (depth % 4, alignment, offsets beyond 32 bits, too few units) stay on k_gemm.
//   k_scatter_mean   grad_x[col[p]] += grad_agg[i] / deg(i) (float atomics, whole 16-byte-aligned row segments): the ONE float atomic
//                    of a training step, so the one place where a step's bits depend on the order in which waves arrive
//   k_scatter_sum_det  the same sums without atomics, for sage_set_deterministic(1): an inverted index of the block (k_det_clear,
//                    k_det_index, k_det_scan: det_index.h's counting sort in the scratch buffer) and one wave per (source row, 256-column slab)
//                    that adds the row's contributions in ascending destination order; also sage_scatter_mean_det on its own
//   (aggregate.hip)  k_gather_reduce / k_scatter_ordered: sum and max aggregation in the gather's and the scatter's place (sage_conv_*_aggr below)
//   k_colsum_*       grad_bias, two deterministic stages
//   k_gemm_dual, k_scatter_and_finals / k_bwd_finals   a small layer's backward pass in two launches: blocks of the kernels above as roles
//                    of one grid (a body that is both a kernel and a role is written once, as a *_block function)
// Host side: forward_plan / backward_plan decide which kernels a layer runs -- the backward pass as an ordered list of steps that
// conv_backward_impl walks to launch and sage_backward_kernel_name walks to print; backward_scratch lays out its scratch buffer for the
// size queries and the launcher alike; a plain-tile product is a GemmArgs, launched as launch_gemm(problem, tile, layouts, stream).
#include <cstring>
#include <mutex>

#include "aggregate.h"
#include "det_index.h"
#include "gemm_streamk_tn.h"
#include "gemm_tile16.h"
#include "side_copy.h"

namespace pope {

// ------------------------------------------------------------------------------------------------
// neighbour gather + mean
// ------------------------------------------------------------------------------------------------
// n_id != nullptr (indexed mode): x is the WHOLE feature matrix and block-local source j lives in row n_id[j]
// (convert_batch's x = data.x[n_id], main.py:118-123, never materialised); destination i's own row goes to x_dst[i].
__device__ __forceinline__ long long src_row(int j, const long long *__restrict__ n_id) { return n_id ? n_id[j] : (long long)j; }

template <bool VEC>
__global__ __launch_bounds__(256) void k_gather_mean(const int *__restrict__ rowptr, const int *__restrict__ col,
                                                     int n_dst, const float *__restrict__ x, int C,
                                                     float *__restrict__ agg, const long long *__restrict__ n_id,
                                                     float *__restrict__ x_dst, const int *__restrict__ n_dst_dev) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    n_dst = dyn_extent(n_dst_dev, n_dst);
    for (int i = wave; i < n_dst; i += nwaves) {
        const int beg = rowptr[i], end = rowptr[i + 1];
        const float inv = end > beg ? 1.0f / (float)(end - beg) : 0.0f;
        if (VEC) {
            const int C4 = C >> 2;
            for (int q = lane; q < C4; q += 64) {
                float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
                int p = beg;
                for (; p + 3 < end; p += 4) {                              // four neighbour rows in flight
                    const long long j0 = src_row(col[p], n_id), j1 = src_row(col[p + 1], n_id), j2 = src_row(col[p + 2], n_id), j3 = src_row(col[p + 3], n_id);
                    const float4 a = reinterpret_cast<const float4 *>(x + (size_t)j0 * C)[q];
                    const float4 b = reinterpret_cast<const float4 *>(x + (size_t)j1 * C)[q];
                    const float4 c = reinterpret_cast<const float4 *>(x + (size_t)j2 * C)[q];
                    const float4 d = reinterpret_cast<const float4 *>(x + (size_t)j3 * C)[q];
                    s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
                    s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
                    s.x += c.x; s.y += c.y; s.z += c.z; s.w += c.w;
                    s.x += d.x; s.y += d.y; s.z += d.z; s.w += d.w;
                }
                for (; p < end; ++p) {
                    const float4 a = reinterpret_cast<const float4 *>(x + (size_t)src_row(col[p], n_id) * C)[q];
                    s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
                }
                s.x *= inv; s.y *= inv; s.z *= inv; s.w *= inv;
                reinterpret_cast<float4 *>(agg + (size_t)i * C)[q] = s;
                if (x_dst) reinterpret_cast<float4 *>(x_dst + (size_t)i * C)[q] = reinterpret_cast<const float4 *>(x + (size_t)n_id[i] * C)[q];
            }
        } else {
            for (int c = lane; c < C; c += 64) {
                float s = 0.f;
                for (int p = beg; p < end; ++p) s += x[(size_t)src_row(col[p], n_id) * C + c];
                agg[(size_t)i * C + c] = s * inv;
                if (x_dst) x_dst[(size_t)i * C + c] = x[(size_t)n_id[i] * C + c];
            }
        }
    }
}

// grad_x[col[p], :] += grad_agg[i, :] / deg(i).  One wave per (destination row, 256-column slab): the row's neighbour
// ids are loaded once, 64 at a time, and broadcast with shuffles, and the slab's four gradient values per lane are in
// registers before the first atomic -- the loop issues nothing but no-return atomics (256 contiguous bytes per wave
// instruction), instead of a dependent col[p] load in front of every one (38 us -> see DESIGN.md §7).
__device__ __forceinline__ void scatter_mean_block(const int *__restrict__ rowptr, const int *__restrict__ col, int n_dst,
                                                   const float *__restrict__ gagg, int C, float *__restrict__ gx,
                                                   const int *__restrict__ n_dst_dev, const int block, const int nblocks) {
    const int lane = threadIdx.x & 63;
    const int wave = (block * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (nblocks * blockDim.x) >> 6;
    const int slabs = (C + 255) / 256;
    n_dst = dyn_extent(n_dst_dev, n_dst);
    for (int w = wave; w < n_dst * slabs; w += nwaves) {
        const int i = w / slabs, c0 = (w - i * slabs) * 256;
        const int beg = rowptr[i], end = rowptr[i + 1];
        if (end == beg) continue;
        const float inv = 1.0f / (float)(end - beg);
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + k * 64 + lane;
            g[k] = c < C ? gagg[(size_t)i * C + c] * inv : 0.f;
        }
        for (int p0 = beg; p0 < end; p0 += 64) {
            const int mine = p0 + lane < end ? col[p0 + lane] : 0;
            const int cnt = min(64, end - p0);
            for (int p = 0; p < cnt; ++p) {
                float *row = gx + (size_t)__shfl(mine, p) * C;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = c0 + k * 64 + lane;
                    if (c < C) atomicAdd(&row[c], g[k]);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_scatter_mean(const int *__restrict__ rowptr, const int *__restrict__ col,
                                                      int n_dst, const float *__restrict__ gagg, int C,
                                                      float *__restrict__ gx, const int *__restrict__ n_dst_dev) {
    scatter_mean_block(rowptr, col, n_dst, gagg, C, gx, n_dst_dev, blockIdx.x, gridDim.x);
}

// x[r, :] = 0 for r in [r0, r1): the rows of grad_x that only the scatter adds to.  Block b of nb: a kernel of its own (k_zero_rows) or
// a role of k_gemm_dual.
__device__ __forceinline__ void zero_rows_block(float *__restrict__ x, int C, int r0, int r1, int b, int nb) {
    if (r1 <= r0) return;
    const size_t n = (size_t)(r1 - r0) * C;
    const size_t stride = (size_t)nb * blockDim.x;
    float *base = x + (size_t)r0 * C;
    const size_t i = (size_t)b * blockDim.x + threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(base) & 15) == 0) {
        const size_t n4 = n >> 2;
        for (size_t q = i; q < n4; q += stride) reinterpret_cast<float4 *>(base)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (size_t q = (n4 << 2) + i; q < n; q += stride) base[q] = 0.f;
    } else {
        for (size_t q = i; q < n; q += stride) base[q] = 0.f;
    }
}

// Both bounds may live on the device.
__global__ __launch_bounds__(256) void k_zero_rows(float *__restrict__ x, int C, int r0, int r1, const int *__restrict__ r0_dev,
                                                   const int *__restrict__ r1_dev) {
    zero_rows_block(x, C, dyn_extent(r0_dev, r0), dyn_extent(r1_dev, r1), blockIdx.x, gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// Deterministic mode (sage_set_deterministic): the scatter as a per-source sum in a fixed order -- no float atomics.
// ------------------------------------------------------------------------------------------------
// An inverted index of the block is built in the scratch buffer -- for every source the destinations that list it -- and one wave
// per (source row, 256-column slab) adds their grad_agg rows in ascending destination order (include/graphpope_hip.h,
// sage_scatter_mean_det: the contract).  The build is det_index.h's counting sort (k_det_clear, k_det_index<false>, k_det_scan,
// k_det_index<true>), and the wave that sums a list sorts it first.  A destination that lists a source twice appears twice with equal
// terms, so ordering by destination is ordering by slot.  Every index read from the block is range-checked: a bad col or rowptr
// entry is skipped, never followed.
int g_sage_deterministic = 0;          // sage_set_deterministic: read by backward_plan, the size queries and sage_eval_metrics (epilogue.hip)

constexpr int DET_AHEAD = 8;

__global__ __launch_bounds__(256) void k_det_clear(int *__restrict__ start, int n_src, const int *__restrict__ n_src_dev) {
    det_clear_body(start, dyn_extent(n_src_dev, n_src), (long long)blockIdx.x * blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
}

// The producer of det_index.h's slots.  FILL = false: start[j] = slots that name source j.  FILL = true (start[j] = first entry of j's
// list): every destination row puts itself into the lists of its sources.
template <bool FILL>
__global__ __launch_bounds__(256) void k_det_index(const int *__restrict__ rowptr, const int *__restrict__ col, int n_dst, int n_src, int nnz,
                                                   int *__restrict__ start, int *__restrict__ list, const int *__restrict__ n_dst_dev,
                                                   const int *__restrict__ n_src_dev) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    n_dst = dyn_extent(n_dst_dev, n_dst);
    n_src = dyn_extent(n_src_dev, n_src);
    for (int i = wave; i < n_dst; i += nwaves) {
        const int beg = max(rowptr[i], 0), end = min(rowptr[i + 1], nnz);
        for (int p = beg + lane; p < end; p += 64) {
            const int j = col[p];
            if ((unsigned)j >= (unsigned)n_src) continue;
            const int at = atomicAdd(&start[j], 1);
            if (FILL && at >= 0 && at < nnz) list[at] = i;
        }
    }
}

__global__ __launch_bounds__(DET_SCAN_THREADS) void k_det_scan(int *__restrict__ start, int n_src, const int *__restrict__ n_src_dev) {
    det_scan_body(start, dyn_extent(n_src_dev, n_src));
}

// acc += grad_agg[i] / deg(i) for the `cnt` destinations i the lanes hold in `ids` (lane t: the t-th), strictly in lane order: the
// product rounded, then added.  DET_AHEAD rows are loaded before the first addition of a round.
// (hipcc's default -ffp-contract=fast would fuse the two into one fma -- also through HIP's __fmul_rn / __fadd_rn, which are plain
// operators compiled under it: contraction is off for this function and the operators are written out.)
#pragma clang fp contract(off)
template <bool VEC>
__device__ __forceinline__ void det_add_rows(const int ids, const int cnt, const int *__restrict__ rowptr, const float *__restrict__ gagg,
                                             const int C, const int c0, const int lane, float (&acc)[4]) {
    float inv = 0.f;
    if (lane < cnt) inv = __fdiv_rn(1.0f, (float)(rowptr[ids + 1] - rowptr[ids]));
    for (int t0 = 0; t0 < cnt; t0 += DET_AHEAD) {
        float r[DET_AHEAD][4], iv[DET_AHEAD];
#pragma unroll
        for (int u = 0; u < DET_AHEAD; ++u) {                       // past the end: the last row again, loaded and not added
            const int t = min(t0 + u, cnt - 1);
            const float *row = gagg + (size_t)__shfl(ids, t) * C;
            iv[u] = __shfl(inv, t);
            if (VEC) {
                const int c = c0 + 4 * lane;
                const float4 q = c < C ? *reinterpret_cast<const float4 *>(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
                r[u][0] = q.x; r[u][1] = q.y; r[u][2] = q.z; r[u][3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = c0 + k * 64 + lane;
                    r[u][k] = c < C ? row[c] : 0.f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < DET_AHEAD; ++u) {
            if (t0 + u < cnt) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float prod = r[u][k] * iv[u];             // plain operators: under contract(off) they carry no 'contract' flag
                    acc[k] = acc[k] + prod;
                }
            }
        }
    }
}
#pragma clang fp contract(fast)

// grad_x[j] = (j < n_dst ? grad_x[j] : 0) + sum over j's list, in ascending destination order, of grad_agg[i] / deg(i).  One wave per
// (source row, 256-column slab).  A list of up to 64 entries is sorted in registers.  A longer one is ranked entry by entry against
// the whole list (quadratic: hub rows are a known cost) into `sorted`, by the wave of slab 0, which then sums every slab
// of the row so that no second wave waits for the sorted list.
template <bool VEC>
__global__ __launch_bounds__(256) void k_scatter_sum_det(const int *__restrict__ rowptr, const int *__restrict__ start, const int *__restrict__ list,
                                                         int *sorted, int n_dst, int n_src, int nnz, const float *__restrict__ gagg, int C,
                                                         float *gx, const int *__restrict__ n_dst_dev, const int *__restrict__ n_src_dev) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int slabs = (C + 255) / 256;
    n_dst = dyn_extent(n_dst_dev, n_dst);
    n_src = dyn_extent(n_src_dev, n_src);
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
            if ((unsigned)ids >= (unsigned)n_dst) ids = 0;          // (the lanes past the list; a list holds destinations only)
            det_row_begin<VEC>(gx, j, keep, C, slab * 256, lane, acc);
            det_add_rows<VEC>(ids, len, rowptr, gagg, C, slab * 256, lane, acc);
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
            if (e < len) sorted[beg + rank] = mine;
        }
        __threadfence();                                            // the wave reads back what its other lanes wrote
        for (int s = 0; s < slabs; ++s) {
            det_row_begin<VEC>(gx, j, keep, C, s * 256, lane, acc);
            for (int p0 = 0; p0 < len; p0 += 64) {
                const int cnt = min(64, len - p0);
                int ids = lane < cnt ? sorted[beg + p0 + lane] : 0;
                if ((unsigned)ids >= (unsigned)n_dst) ids = 0;
                det_add_rows<VEC>(ids, cnt, rowptr, gagg, C, s * 256, lane, acc);
            }
            det_row_end<VEC>(gx, j, C, s * 256, lane, acc);
        }
    }
}

// Column sums in two deterministic stages: part[s][c] = sum over row slice s, then out[c] = sum_s part[s][c].
constexpr int COLSUM_SPLITS = 256;

// VEC: lane l owns 4 adjacent columns (16-byte loads, a wave covers 256 columns of a row); else one column per lane.
// (bx, by) of (gx, gy): the block's place in the launch -- a kernel of its own (k_colsum_partial) or a role of k_gemm_dual.
template <bool VEC>
__device__ __forceinline__ void colsum_partial_block(const float *__restrict__ g, int rows, int C, float *__restrict__ part, int bx, int by, int gy) {
    constexpr int W = VEC ? 4 : 1;
    __shared__ float red[4][64 * W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = (bx * 64 + lane) * W;
    const int per = (rows + gy - 1) / gy;
    const int r0 = by * per, r1 = min(rows, r0 + per);
    float s[W];
#pragma unroll
    for (int k = 0; k < W; ++k) s[k] = 0.f;
    if (c < C) {
        // four rows requested before the first is added (round 4: one load per trip compiled to load - wait - add, a wave's ten
        // rows ten serial round trips); the additions keep their order, so the sums keep their bits
        int i = r0 + wave;
        for (; i + 12 < r1; i += 16) {
            if constexpr (VEC) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4 *>(g + (size_t)(i + 4 * u) * C + c);
#pragma unroll
                for (int u = 0; u < 4; ++u) { s[0] += v[u].x; s[1] += v[u].y; s[2] += v[u].z; s[3] += v[u].w; }
            } else {
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = g[(size_t)(i + 4 * u) * C + c];
#pragma unroll
                for (int u = 0; u < 4; ++u) s[0] += v[u];
            }
        }
        for (; i < r1; i += 4) {
            if constexpr (VEC) {
                const float4 v = *reinterpret_cast<const float4 *>(g + (size_t)i * C + c);
                s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
            } else {
                s[0] += g[(size_t)i * C + c];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) red[wave][lane * W + k] = s[k];
    __syncthreads();
    if (wave == 0 && c < C)
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int j = lane * W + k;
            part[(size_t)by * C + c + k] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
        }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_colsum_partial(const float *__restrict__ g, int rows, int C, float *__restrict__ part,
                                                        const int *__restrict__ rows_dev) {
    colsum_partial_block<VEC>(g, dyn_extent(rows_dev, rows), C, part, blockIdx.x, blockIdx.y, gridDim.y);
}

// 16 columns x 16 split-groups per block: a one-thread-per-column loop over the 64 partials is 64 dependent-latency
// loads (15 us measured); here every thread adds 4 and LDS folds the 16 groups in a fixed order.
__global__ __launch_bounds__(256) void k_colsum_final(const float *__restrict__ part, int splits, int C, float *__restrict__ out) {
    colsum_final_block(part, splits, C, out, blockIdx.x);            // (gemm_streamk_tn.h: also a role of the weight gradients' fix-up launch)
}

// The first stage over C columns as (column groups, row slices): the grid of k_colsum_partial, the shape of the role in k_gemm_dual.
static dim3 colsum_partial_grid(int C, bool vec) { return dim3(vec ? (C + 255) / 256 : (C + 63) / 64, COLSUM_SPLITS); }

static void enqueue_colsum_partial(const float *g, int rows, int C, float *part, const int *rows_dev, bool vec, hipStream_t stream) {
    if (vec) hipLaunchKernelGGL(k_colsum_partial<true>, colsum_partial_grid(C, true), dim3(256), 0, stream, g, rows, C, part, rows_dev);
    else hipLaunchKernelGGL(k_colsum_partial<false>, colsum_partial_grid(C, false), dim3(256), 0, stream, g, rows, C, part, rows_dev);
}

// ------------------------------------------------------------------------------------------------
// f32 MFMA GEMM (tile machinery in gemm_tile.h)
// ------------------------------------------------------------------------------------------------
// C[M, N] = sum_{p < 2} A_p[M, K_p] * B_p[N, K_p]^T (+ bias[n]).  grid = (ceil(M/TM), ceil(N/TN), splits).
// splits > 1: every z handles a slice of the depth of every product and writes its partial tile to
// slab[z][M][N]; k_slab_reduce adds them (fixed order: deterministic).
// Twin mode (twin.tiles_n > 0): TWO results that share the A operand, C = A0 * B0^T and twin.C = A0 * twin.B^T, in one
// launch -- grid.y covers the tile columns of both (the weight gradients of lin_l and lin_r both multiply grad_out^T;
// grad_x and grad_agg both multiply grad_out): twice the blocks per launch, half the split-K slabs, one launch less.
struct Twin {
    Operand B;
    float *C;
    int tiles_n;               // tile columns of the first result; 0 = plain GEMM
};

// One product, as the host describes it (gemm_problem and assignments by name) and as the kernels take it.
struct GemmArgs {
    Operand A0, B0;
    int K0;
    Operand A1, B1;
    int K1, M, N;
    const float *bias;
    float *C;
    long long ldc;
    float *slab;
    Twin twin;
    const int *m_dev, *k0_dev;     // device extents (null: the host-side size is the size): the true M, the true depth of product 0
    int gx, gy, gz;                // the launch shape: row tiles, column tiles (x2 in twin mode) -- filled per tile by gemm_set_grid -- and splits
};

// One block of a planned GEMM: tile (bx, by), split bz.
template <int TM, int TN, int WM, int WN, int LA, int LB>
__device__ __forceinline__ void gemm_block(GemmArgs p, int bx, int by, int z, float *As, float *Bs) {
    constexpr int NT = TN / WN / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int splits = p.gz;
    // device extents: the true row count / the true depth of product 0 (the launch covers the capacities).  The slab
    // stride stays the capacity M: k_slab_reduce is given the same.
    const int M_cap = p.M;
    const int M = dyn_extent(p.m_dev, p.M), N = p.N, K0 = dyn_extent(p.k0_dev, p.K0), K1 = p.K1;
    if (bx * TM >= M) return;
    Operand B0 = p.B0;
    float *C = p.C, *slab = p.slab;
    if (p.twin.tiles_n > 0 && by >= p.twin.tiles_n) {       // second result: its own B, C and slab region
        by -= p.twin.tiles_n;
        B0 = p.twin.B;
        C = p.twin.C;
        slab += (size_t)splits * M_cap * N;
    }
    const int m0 = bx * TM, n0 = by * TN;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    // depth range of this split inside each product, in whole LDS stages
    const int per0 = K0 > 0 ? ((K0 + splits - 1) / splits + GK - 1) / GK * GK : 0;
    const int per1 = K1 > 0 ? ((K1 + splits - 1) / splits + GK - 1) / GK * GK : 0;
    const int kb0 = z * per0, ke0 = min(K0, kb0 + per0), kb1 = z * per1, ke1 = min(K1, kb1 + per1);
    mfma_accumulate<TM, TN, WM, WN, LA, LB>(acc, p.A0, B0, kb0, ke0, p.A1, p.B1, kb1, ke1, m0, n0, M, N, As, Bs);
    // C/D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float *dst = splits > 1 ? slab + (size_t)z * M_cap * N : C;
    const long long ld = splits > 1 ? (long long)N : p.ldc;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = n0 + wn * (TN / WN) + t * 32 + (lane & 31);
        if (n >= N) continue;
        const float b = (p.bias && splits == 1) ? p.bias[n] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m < M) dst[(size_t)m * ld + n] = acc[t][r] + b;
        }
    }
}

template <int TM, int TN, int WM, int WN, int LA, int LB>
__global__ __launch_bounds__(256) void k_gemm(GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *As = reinterpret_cast<float *>(smem);
    gemm_block<TM, TN, WM, WN, LA, LB>(p, blockIdx.x, blockIdx.y, blockIdx.z, As, As + Tile<TM>::FLOATS);
}

// Four independent pieces of a small layer's backward pass that only share grad_out, as ONE launch (sage_conv_backward):
//   blocks [0, n0)            grad_x[:n_dst] = grad_out * W_r  and  grad_agg = grad_out * W_l   (twin GEMM p0, operands KC x OC)
//   blocks [n0, n0 + n1)      the split-K slabs of grad_w_l / grad_w_r                          (twin GEMM p1, operands OC x OC)
//   the next zero_blocks      grad_x[n_dst : n_src] = 0 (the rows only the scatter adds to)
//   the last cs_gx * cs_gy    partial column sums of grad_out (the bias gradient)
// Each of them alone is a 5-13 us launch of ~200 blocks that leaves half the chip idle: 36 us in sequence, one launch together.
struct DualAux {
    float *zero_x;                 // grad_x, or null
    int zero_C, zero_r0, zero_r1;
    const int *zero_r0_dev, *zero_r1_dev;
    int zero_blocks;
    const float *cs_g;             // grad_out for the column sums, or null
    int cs_rows, cs_C;
    float *cs_part;
    const int *cs_rows_dev;
    int cs_gx, cs_gy;
};

template <int TM, int TN, int WM, int WN>
__global__ __launch_bounds__(256) void k_gemm_dual(GemmArgs p0, GemmArgs p1, DualAux aux) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *As = reinterpret_cast<float *>(smem), *Bs = As + Tile<TM>::FLOATS;
    int b = blockIdx.x;
    const int n0 = p0.gx * p0.gy * p0.gz, n1 = p1.gx * p1.gy * p1.gz;
    if (b < n0) {
        gemm_block<TM, TN, WM, WN, LAYOUT_KC_VEC, LAYOUT_OC_VEC>(p0, b % p0.gx, (b / p0.gx) % p0.gy, b / (p0.gx * p0.gy), As, Bs);
        return;
    }
    b -= n0;
    if (b < n1) {
        gemm_block<TM, TN, WM, WN, LAYOUT_OC_VEC, LAYOUT_OC_VEC>(p1, b % p1.gx, (b / p1.gx) % p1.gy, b / (p1.gx * p1.gy), As, Bs);
        return;
    }
    b -= n1;
    if (b < aux.zero_blocks) {
        zero_rows_block(aux.zero_x, aux.zero_C, dyn_extent(aux.zero_r0_dev, aux.zero_r0), dyn_extent(aux.zero_r1_dev, aux.zero_r1), b, aux.zero_blocks);
        return;
    }
    b -= aux.zero_blocks;
    if (aux.cs_g) colsum_partial_block<true>(aux.cs_g, dyn_extent(aux.cs_rows_dev, aux.cs_rows), aux.cs_C, aux.cs_part, b % aux.cs_gx, b / aux.cs_gx, aux.cs_gy);
}

// C[i / N][i % N] = sum over z of slab[z][i], z ascending, for the `elems` elements of a result; results = 2 in twin mode: the second
// result's slabs follow the first's and go to C2.  Block `block` of `nblocks`: k_slab_reduce, or the first role of bwd_finals_block.
__device__ __forceinline__ void slab_reduce_block(const float *__restrict__ slab, int splits, size_t elems, int N, float *__restrict__ C,
                                                  float *__restrict__ C2, int results, long long ldc, int block, int nblocks) {
    for (size_t t = (size_t)block * blockDim.x + threadIdx.x; t < elems * results; t += (size_t)nblocks * blockDim.x) {
        const int which = t >= elems;
        const size_t i = t - (which ? elems : 0);
        const float *src = slab + (size_t)which * splits * elems + i;
        float s = 0.f;
#pragma unroll 4
        for (int z = 0; z < splits; ++z) s += src[(size_t)z * elems];
        (which ? C2 : C)[(i / N) * ldc + (i % N)] = s;
    }
}

__global__ __launch_bounds__(256) void k_slab_reduce(const float *__restrict__ slab, int splits, size_t elems, int N,
                                                     float *__restrict__ C, float *__restrict__ C2, int results, long long ldc) {
    slab_reduce_block(slab, splits, elems, N, C, C2, results, ldc, blockIdx.x, gridDim.x);
}

// C [M, N] (row stride ldc) = A * B^T over depth K in one pass.  Everything else a product may have is assigned by name: a second product
// (A1, B1, K1), bias, a twin result (twin.B, twin.C), depth splits with their slab (gz, slab), device extents (m_dev, k0_dev).
static GemmArgs gemm_problem(const Operand &A, const Operand &B, int K, int M, int N, float *C, long long ldc) {
    GemmArgs p{};
    p.A0 = A; p.B0 = B; p.K0 = K; p.M = M; p.N = N; p.C = C; p.ldc = ldc; p.gz = 1;
    return p;
}

// The launch shape of a problem under TM x TN tiles.
static void gemm_set_grid(GemmArgs &p, int TM, int TN) {
    const int tiles_n = (p.N + TN - 1) / TN;
    p.twin.tiles_n = p.twin.C ? tiles_n : 0;
    p.gx = (p.M + TM - 1) / TM; p.gy = p.twin.C ? 2 * tiles_n : tiles_n;
}

// The two reductions behind k_gemm_dual in one launch: blocks [0, reduce_blocks) add the split-K slabs of both weight
// gradients, the rest fold the partial column sums of the bias gradient (k_colsum_final's block shape).
// (colsum_final_block: gemm_streamk_tn.h)
struct BwdFinals {
    const float *slab;
    int splits;
    size_t elems;
    int N;
    float *C, *C2;
    long long ldc;
    int reduce_blocks;
    const float *cs_part;
    int cs_splits, cs_C;
    float *cs_out;
};

__device__ __forceinline__ void bwd_finals_block(const BwdFinals &f, const int block) {
    if (block < f.reduce_blocks) {
        slab_reduce_block(f.slab, f.splits, f.elems, f.N, f.C, f.C2, 2, f.ldc, block, f.reduce_blocks);
        return;
    }
    colsum_final_block(f.cs_part, f.cs_splits, f.cs_C, f.cs_out, block - f.reduce_blocks);
}

__global__ __launch_bounds__(256) void k_bwd_finals(BwdFinals f) { bwd_finals_block(f, (int)blockIdx.x); }

// The scatter of grad_agg and the two reductions behind k_gemm_dual read nothing of one another: one launch, the (few, short)
// reduction blocks first.
__global__ __launch_bounds__(256) void k_scatter_and_finals(const int *__restrict__ rowptr, const int *__restrict__ col, int n_dst,
                                                            const float *__restrict__ gagg, int C, float *__restrict__ gx,
                                                            const int *__restrict__ n_dst_dev, BwdFinals f, int finals_blocks) {
    if ((int)blockIdx.x < finals_blocks) bwd_finals_block(f, (int)blockIdx.x);
    else scatter_mean_block(rowptr, col, n_dst, gagg, C, gx, n_dst_dev, (int)blockIdx.x - finals_blocks, (int)gridDim.x - finals_blocks);
}

template <int TM, int TN, int WM, int WN, int LA, int LB>
static int launch_gemm_layout(const GemmArgs &p, hipStream_t stream) {
    const size_t lds = tile_lds_bytes<TM, TN>();
    static LdsOptIn opt_in;
    if (!opt_in.done()) {
        POPE_HIP(hipFuncSetAttribute((const void *)k_gemm<TM, TN, WM, WN, LA, LB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        opt_in.mark();
    }
    hipLaunchKernelGGL((k_gemm<TM, TN, WM, WN, LA, LB>), dim3(p.gx, p.gy, p.gz), dim3(256), lds, stream, p);
    return POPE_OK;
}

// Operand layouts are compile-time (gemm_tile.h): the three combinations SAGEConv produces get straight-line vector
// prefetch code, anything else the generic kernel.
struct GemmLayouts { Layout a, b; };

// The instantiation for operands of these layouts (a0 / b0: product 0; a1 / b1: product 1 if `second`; tb: the twin's B if `twin`).
static GemmLayouts gemm_layouts(Layout a0, Layout b0, bool second, Layout a1, Layout b1, bool twin, Layout tb) {
    Layout la = a0, lb = b0;
    if (second && (a1 != la || b1 != lb)) la = lb = LAYOUT_GENERIC;
    if (twin && tb != lb) la = lb = LAYOUT_GENERIC;
    if ((la == LAYOUT_KC_VEC || la == LAYOUT_OC_VEC) && lb == la) return {la, lb};
    if (la == LAYOUT_KC_VEC && lb == LAYOUT_OC_VEC) return {la, lb};
    return {LAYOUT_GENERIC, LAYOUT_GENERIC};
}

template <int TM, int TN, int WM, int WN>
static int launch_gemm_tile(GemmArgs p, GemmLayouts l, hipStream_t stream) {
    gemm_set_grid(p, TM, TN);
    if (l.a == LAYOUT_KC_VEC && l.b == LAYOUT_KC_VEC) return launch_gemm_layout<TM, TN, WM, WN, LAYOUT_KC_VEC, LAYOUT_KC_VEC>(p, stream);
    if (l.a == LAYOUT_OC_VEC && l.b == LAYOUT_OC_VEC) return launch_gemm_layout<TM, TN, WM, WN, LAYOUT_OC_VEC, LAYOUT_OC_VEC>(p, stream);
    if (l.a == LAYOUT_KC_VEC && l.b == LAYOUT_OC_VEC) return launch_gemm_layout<TM, TN, WM, WN, LAYOUT_KC_VEC, LAYOUT_OC_VEC>(p, stream);
    return launch_gemm_layout<TM, TN, WM, WN, LAYOUT_GENERIC, LAYOUT_GENERIC>(p, stream);
}

// Diagnostic knobs behind pope_debug_set() (abi.cpp), declared in common.h.
int g_sage_forward_overlap = 1;        // POPE_KNOB_SAGE_FORWARD_OVERLAP: 1 (default) gather beside half of the projection, 0 one after the other
int g_forward_whole_tiles = 1;         // POPE_KNOB_FORWARD_WHOLE_TILES: 0 = forward projection without the kernels of gemm_tile16.h
int g_gemm_tile16_buffers = 4;         // POPE_KNOB_GEMM_TILE16_BUFFERS
int g_streamk_xcd = 1;                 // POPE_KNOB_STREAMK_XCD

static long long tiles(int M, int N, int tm, int tn) { return (long long)((M + tm - 1) / tm) * ((N + tn - 1) / tn); }

// Tile choice: the largest tile that still gives every CU about two blocks (2 x 256 = 512): co-resident blocks overlap
// one block's staging waits with another's MFMAs, and many small blocks balance better over 256 CUs than 1.2 per CU.
struct GemmTile { int tm, tn; };
static GemmTile gemm_tile_for(int M, int N, int splits, int results) {
    if (tiles(M, N, 128, 256) * splits * results >= 512) return {128, 256};
    if (tiles(M, N, 64, 128) * splits * results >= 384) return {64, 128};
    return {64, 64};
}

// k_gemm over the problem in this tile and these layouts, and behind it k_slab_reduce if the depth is split.
static int launch_gemm(const GemmArgs &p, GemmTile tile, GemmLayouts layouts, hipStream_t stream) {
    const int rc = tile.tm == 128   ? launch_gemm_tile<128, 256, 4, 1>(p, layouts, stream)
                   : tile.tn == 128 ? launch_gemm_tile<64, 128, 2, 2>(p, layouts, stream)
                                    : launch_gemm_tile<64, 64, 2, 2>(p, layouts, stream);
    if (rc) return rc;
    const int results = p.twin.C ? 2 : 1;
    if (p.gz > 1)
        hipLaunchKernelGGL(k_slab_reduce, dim3(capped_grid((size_t)p.M * p.N * results, 256)), dim3(256), 0, stream, p.slab, p.gz,
                           (size_t)p.M * p.N, p.N, p.C, p.twin.C, results, p.ldc);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

// Weight gradients reduce over the n_dst rows: split that depth so the 64 x 128 tiles give ~400 blocks
// (measured: 85 us per gradient at 756 x 256 x 10 000 against 148 us with 64 x 64 tiles and fewer, longer splits).
static int weight_grad_splits(int64_t n_dst, int c_in, int c_out) {
    const long long t = 2 * tiles(c_out, c_in, 64, 128);            // both weight gradients in one twin launch
    int s = (int)((400 + t - 1) / t);
    const int max_s = (int)((n_dst + 4 * GK - 1) / (4 * GK));       // at least four LDS stages of depth per block
    if (s > max_s) s = max_s;
    return s < 1 ? 1 : s;
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- forward projection as a stream-K launch (gemm_streamk.h) ----
constexpr int SK_MAX_GRID = 256;                     // one persistent block per CU of an MI355X

static bool streamk_shape_ok(int64_t M, int32_t K0, int32_t K1, int32_t N) {
    if ((K0 & 3) || (K1 & 3) || M <= 0 || N <= 0) return false;
    const long long tiles = ((M + SK_TM - 1) / SK_TM) * ((N + SK_TN - 1) / SK_TN);
    const long long S = (K0 + SK_GK - 1) / SK_GK + (K1 + SK_GK - 1) / SK_GK;
    return tiles * S >= 4ll * SK_MAX_GRID;           // enough work (in depth-32 units) for every block to amortise its partial tiles
}

// &g_sk_zero (lds_dma.h) on the current device: the source of the loaders' depth padding.
static int sk_zero_page(const float **zero) {
    static const float *page[64];
    int dev = 0;
    POPE_HIP(hipGetDevice(&dev));
    POPE_REQUIRE(dev >= 0 && dev < 64, "device index %d out of range", dev);
    if (!page[dev]) POPE_HIP(hipGetSymbolAddress((void **)&page[dev], HIP_SYMBOL(g_sk_zero)));
    *zero = page[dev];
    return POPE_OK;
}

// One persistent block per CU, fewer if there are fewer units (T) than that.
static int streamk_grid(int cus, long long T) { return (int)std::min<long long>(std::min(cus, SK_MAX_GRID), T); }

static long long streamk_units(int M, int N, int K0, int K1) {
    return tiles(M, N, SK_TM, SK_TN) * ((K0 + SK_GK - 1) / SK_GK + (K1 + SK_GK - 1) / SK_GK);
}

// out = A0 * B0^T + A1 * B1^T + bias through k_gemm_streamk_ld + k_streamk_fixup.  The caller has checked that the product
// qualifies (forward_plan: shape, alignment, 32-bit offsets, a slab of sk_slab_bytes(grid)).
static int gemm_streamk(const float *A0, const float *B0, int K0, const float *A1, const float *B1, int K1, long long lda, long long ldb,
                        int M, int N, const float *bias, float *C, long long ldc, void *slab, int cus, hipStream_t stream,
                        const int *m_dev) {
    SkArgs a;
    a.p[0] = SkProduct{A0, B0, lda, ldb, K0};
    a.p[1] = SkProduct{K1 > 0 ? A1 : A0, K1 > 0 ? B1 : B0, lda, ldb, K1};
    a.M = M; a.N = N; a.bias = bias; a.C = C; a.ldc = ldc; a.slab = (float *)slab;
    a.tiles_m = (M + SK_TM - 1) / SK_TM; a.tiles_n = (N + SK_TN - 1) / SK_TN;
    a.S0 = (K0 + SK_GK - 1) / SK_GK; a.S1 = (K1 + SK_GK - 1) / SK_GK;
    a.m_dev = m_dev;
    const int grid = streamk_grid(cus, streamk_units(M, N, K0, K1));
    static LdsOptIn opt_in;
    if (!opt_in.done()) {
        POPE_HIP(hipFuncSetAttribute((const void *)k_gemm_streamk_ld<SK_GK>, hipFuncAttributeMaxDynamicSharedMemorySize, SkStage<SK_GK>::LDS_BYTES));
        opt_in.mark();
    }
    int rc;
    if ((rc = sk_zero_page(&a.zero))) return rc;
    hipLaunchKernelGGL(k_gemm_streamk_ld<SK_GK>, dim3((unsigned)grid), dim3(SKL_THREADS), SkStage<SK_GK>::LDS_BYTES, stream, a);
    hipLaunchKernelGGL(k_streamk_fixup, dim3(a.tiles_m * a.tiles_n, SK_FIX_PARTS), dim3(256), 0, stream, a, grid);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

// ---- forward projection as whole tiles fitted to the chip (gemm_tile16.h): no partial tiles, no fix-up ----
template <int RB, int NBUF>
static int launch_tile16_as(const T16Args &a, int grid, hipStream_t stream) {
    static LdsOptIn opt_in;
    constexpr int lds = T16Shape<RB, NBUF>::LDS_BYTES;
    if (!opt_in.done()) {
        POPE_HIP(hipFuncSetAttribute((const void *)k_gemm_tile16<RB, NBUF>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        opt_in.mark();
    }
    hipLaunchKernelGGL((k_gemm_tile16<RB, NBUF>), dim3((unsigned)grid), dim3(T16_THREADS), lds, stream, a);
    return POPE_OK;
}

// POPE_KNOB_GEMM_TILE16_BUFFERS: 3 or 4 stage buffers (gemm_tile16.h: one or two stage times to hide a request).
static int t16_buffers() { return g_gemm_tile16_buffers == 4 ? 4 : 3; }

template <int RB>
static int launch_tile16(const T16Args &a, int grid, hipStream_t stream) {
    return t16_buffers() == 4 ? launch_tile16_as<RB, 4>(a, grid, stream) : launch_tile16_as<RB, 3>(a, grid, stream);
}

// A whole-tile product ready to launch: arguments, tile height (rb x 16 rows, chosen by forward_plan) and grid.
struct T16Plan {
    T16Args a;
    int rb = 0, grid = 0;
};

static int t16_fill(const float *A0, const float *B0, int K0, const float *A1, const float *B1, int K1, long long lda, long long ldb, int M, int N,
                    const float *bias, float *C, long long ldc, const int *m_dev, int rb, int cus, T16Plan *plan) {
    T16Args &a = plan->a;
    int rc;
    if ((rc = sk_zero_page(&a.zero))) return rc;
    a.p[0] = SkProduct{A0, B0, lda, ldb, K0};
    a.p[1] = SkProduct{K1 > 0 ? A1 : A0, K1 > 0 ? B1 : B0, lda, ldb, K1};
    a.M = M; a.N = N; a.bias = bias; a.C = C; a.ldc = ldc; a.m_dev = m_dev;
    a.rows = nullptr; a.accumulate = 0; a.stat_a = a.stat_b = nullptr;
    a.tiles_m = (M + 16 * rb - 1) / (16 * rb); a.tiles_n = (N + T16_TN - 1) / T16_TN;
    a.S0 = (K0 + T16_GK - 1) / T16_GK; a.S1 = (K1 + T16_GK - 1) / T16_GK;
    plan->grid = a.tiles_n == 2 ? (a.tiles_m + 7) / 8 * 16 : a.tiles_m * a.tiles_n;
    if (m_dev) plan->grid = std::min(plan->grid, a.tiles_n == 2 ? (cus + 15) / 16 * 16 : cus);   // capacity rows: one block per CU walks the true tiles
    plan->rb = rb;
    return POPE_OK;
}

static int t16_launch(const T16Plan &plan, hipStream_t stream) {
    int rc;
    switch (plan.rb) {
    case 1: rc = launch_tile16<1>(plan.a, plan.grid, stream); break;
    case 2: rc = launch_tile16<2>(plan.a, plan.grid, stream); break;
    case 3: rc = launch_tile16<3>(plan.a, plan.grid, stream); break;
    case 4: rc = launch_tile16<4>(plan.a, plan.grid, stream); break;
    case 5: rc = launch_tile16<5>(plan.a, plan.grid, stream); break;
    case 6: rc = launch_tile16<6>(plan.a, plan.grid, stream); break;
    case 7: rc = launch_tile16<7>(plan.a, plan.grid, stream); break;
    default: rc = launch_tile16<8>(plan.a, plan.grid, stream); break;
    }
    if (rc) return rc;
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

// A caller's wish for the first stage of the BatchNorm statistics of the layer's output (main.py:207) out of the projection's epilogue:
// pa / pb [parts_cap, c_out] doubles.  Filled in by the whole-tile kernels only; parts = 0 says "not produced" (the caller then runs
// the statistics pass of sage_bn_relu_dropout_forward as before).
struct BnStatsOut {
    double *pa = nullptr, *pb = nullptr;
    int parts_cap = 0;
    int parts = 0, rows_per_part = 0;      // out
};

// bn_info of the _stats entry points: what the call (status rc) left of the statistics.
static int stats_report(int rc, const BnStatsOut &st, int32_t *bn_info) {
    bn_info[0] = st.parts; bn_info[1] = st.rows_per_part;
    return rc;
}

// The product that leaves the layer's final values in `out` also leaves the statistics, if they are wanted and fit.
static void stats_take(BnStatsOut *st, T16Plan &plan) {
    if (!st || !st->pa || !st->pb || plan.a.tiles_m > st->parts_cap) return;
    plan.a.stat_a = st->pa; plan.a.stat_b = st->pb;
    st->parts = plan.a.tiles_m; st->rows_per_part = 16 * plan.rb;
}

static int gemm_tile16(const float *A0, const float *B0, int K0, const float *A1, const float *B1, int K1, long long lda, long long ldb,
                       int M, int N, const float *bias, float *C, long long ldc, int rb, int cus, hipStream_t stream, const int *m_dev,
                       BnStatsOut *stats) {
    T16Plan plan;
    int rc = t16_fill(A0, B0, K0, A1, B1, K1, lda, ldb, M, N, bias, C, ldc, m_dev, rb, cus, &plan);
    if (rc) return rc;
    stats_take(stats, plan);
    return t16_launch(plan, stream);
}

// ---- which kernels a layer's forward pass runs: decided HERE and nowhere else (no HIP calls) ----
// The projection out = agg W_l^T + b_l + x_dst W_r^T is, in this order of preference:
//   FWD_OVERLAPPED  whole tiles in two launches, the x_dst half beside the gather (forward_overlapped)
//   FWD_TILE16      gather, then whole tiles fitted to the chip in one pass (gemm_tile16.h)
//   FWD_STREAMK     gather, then stream-K (gemm_streamk.h)
//   FWD_PLAIN       gather, then the plain tile kernel (gemm_tile.h), tile tm x tn
// conv_forward_run launches what this says; sage_forward_kernel_name prints it.
enum FwdPath { FWD_OVERLAPPED, FWD_TILE16, FWD_STREAMK, FWD_PLAIN };
struct FwdPlan {
    FwdPath path;
    int rb;                // whole tiles: tile height / 16
    GemmTile tile;         // plain tile kernel
    GemmLayouts layouts;   // ... and its operand layouts
    bool gather_vec;       // every path but the overlapped one: k_gather_mean<true> (16-byte accesses) or <false>
};

// 16-byte alignment of the operands: x = the matrix the rows are gathered from, own = the matrix the one-pass projection
// reads the destination rows from (x itself, or x_dst), x_dst_out = the x_dst the gather writes is aligned (or absent).
struct FwdAligned { bool x, agg, own, x_dst_out, w_l, w_r; };

// Tile height of a whole-tile product over a_rows x ld operands (0: not these kernels).  Leading dimensions and depths are
// all c_in, so sk_operand_ok is the pointers' alignment (`aligned`) once the depths are multiples of 4.
static int t16_rb(long long a_rows, int M, int N, int K0, int K1, long long ld, bool aligned, int cus, bool small) {
    if (!g_forward_whole_tiles) return 0;
    if ((K0 & 3) || (K1 & 3) || M <= 0 || N <= 0 || K0 <= 0) return 0;
    if (a_rows * ld * 4 >= (1ll << 32) || (long long)N * ld * 4 >= (1ll << 32)) return 0;       // the loaders' 32-bit byte offsets
    if (!aligned) return 0;
    // small = a product that cannot fill the chip whatever the tile: the shortest tiles (16 or 32 rows) that give the most blocks
    return small ? t16_pick_rb(M, N, cus, 0.3, 1) : t16_pick_rb(M, N, cus);
}

// x_rows: rows of the matrix the overlapped path reads the destination rows from; slab_bytes: the stream-K scratch (0: none).
static FwdPlan forward_plan(int64_t n_dst, int32_t c_in, int32_t c_out, int64_t x_rows, int cus, const FwdAligned &al, size_t slab_bytes) {
    const int M = (int)n_dst, N = c_out;
    const bool big = streamk_shape_ok(n_dst, c_in, c_in, c_out);
    // the gather writes agg and, in indexed mode, the destination rows -- which are then `own` (in plain mode own is x itself)
    const bool gather_vec = (c_in & 3) == 0 && al.x && al.agg && al.x_dst_out && al.own;
    if (g_sage_forward_overlap && big && al.x && al.agg && al.x_dst_out) {
        const int first = t16_rb(std::max<long long>(M, x_rows), M, N, c_in, 0, c_in, al.x && al.w_r, cus, false);
        const int second = first ? t16_rb(M, M, N, c_in, 0, c_in, al.agg && al.w_l, cus, false) : 0;
        // taller tiles do not fit the fused kernel's 128 registers (they spill 140-430 bytes per lane)
        if (first && second == first && first <= 5) return {FWD_OVERLAPPED, first, {0, 0}, {LAYOUT_GENERIC, LAYOUT_GENERIC}, true};
    }
    const bool all = al.agg && al.w_l && al.own && al.w_r;
    if (big || (long long)M * N >= 64 * 1024) {                  // (tiny products stay on the plain tile kernel)
        const int rb = t16_rb(M, M, N, c_in, c_in, c_in, all, cus, !big);
        if (rb) return {FWD_TILE16, rb, {0, 0}, {LAYOUT_GENERIC, LAYOUT_GENERIC}, gather_vec};
    }
    if (big && (long long)M * c_in * 4 < (1ll << 32) && (long long)N * c_in * 4 < (1ll << 32) && all &&
        slab_bytes >= sk_slab_bytes(streamk_grid(cus, streamk_units(M, N, c_in, c_in))))
        return {FWD_STREAMK, 0, {0, 0}, {LAYOUT_GENERIC, LAYOUT_GENERIC}, gather_vec};
    // operands as conv_forward_run builds them, all depth-contiguous: agg W_l^T + own W_r^T
    const GemmLayouts layouts = gemm_layouts(pick_layout(al.agg, c_in, 1, M, c_in), pick_layout(al.w_l, c_in, 1, N, c_in), true,
                                             pick_layout(al.own, c_in, 1, M, c_in), pick_layout(al.w_r, c_in, 1, N, c_in), false, LAYOUT_GENERIC);
    return {FWD_PLAIN, 0, gemm_tile_for(M, N, 1, 1), layouts, gather_vec};
}

// ---- layer forward as TWO launches that overlap the gather with half of the projection (round 3) ----
// The gather is HBM-bound (64 us inside the step), the projection MFMA-bound (78 us), and they ran one after the other.
// out = x_dst W_r^T + b does not need the gather: launch 1 carries that product (reading the destination rows straight from
// the source / feature matrix, through n_id in indexed mode) in its first blocks -- one per CU, dispatched first -- and the
// gather in the remaining blocks, which share the CUs with them; launch 2 adds agg W_l^T into out.  No block waits for
// another block.  Every block of launch 1 carries the GEMM role's LDS reservation, so only one or two gather blocks fit a
// CU: the gather role keeps twelve 16-byte loads in flight per lane (k_gather_mean: four) to make up for it.
// (Measured and not kept: x_dst written by the GEMM role out of LDS instead of read + written by the gather role -- by the consumer
//  waves (their copy doubled the fused kernel's spills) or by the loader waves: the launch took 84 us instead of 79 and the step
//  0.332 ms instead of 0.313 either way (128-byte pieces of 3 KB rows, stage by stage, are poor stores); and no x_dst at all, the weight-gradient
//  kernel reading the rows through n_id (sage_conv_backward_indexed): its 1 KB random reads cost 29 us more than the copy.)
struct GatherArgs {
    const int *rowptr, *col;
    int n_dst;
    const float *x;
    int C;
    float *agg;
    const long long *n_id;
    float *x_dst;
    const int *n_dst_dev;
};

// Only one or two of these blocks fit a CU beside the GEMM role's LDS, so what k_gather_mean hides behind occupancy is
// hidden here by a pipeline over the rows of a wave: while row j's data is in flight the wave loads rowptr of row j + 3, the
// neighbour ids of row j + 2 (one coalesced load, a lane per neighbour) and their n_id entries for row j + 1; the data
// phase takes its row addresses from registers (shuffles) and keeps twelve 16-byte loads in flight per lane.  Sums are
// formed in k_gather_mean's order (a short last group re-reads the last neighbour with weight 0: v * 1 and s + v * 0 are
// exact), so agg is bit for bit the same.  Rows with more than 64 neighbours take the plain loop.  (s_setprio 3 for this role:
// measured, no difference.)
__device__ __forceinline__ void gather_role(const GatherArgs &g, const int block, const int nblocks) {
    const int lane = threadIdx.x & 63;
    const int wave = block * (T16_THREADS / 64) + (threadIdx.x >> 6), nwaves = nblocks * (T16_THREADS / 64);
    const int n_dst = dyn_extent(g.n_dst_dev, g.n_dst);
    const int C = g.C, C4 = C >> 2;
    // pipeline registers: row r3 has its rowptr pair requested, r2 its neighbour ids, r1 their source rows, r0 is being summed
    int b1 = 0, e1 = 0, b2 = 0, e2 = 0, c1 = 0;
    long long id0 = 0, own0 = 0;
    int b0 = 0, e0 = 0;
    auto rowptr_pair = [&](int i, int &b, int &e) {
        if (i < n_dst) { b = g.rowptr[i]; e = g.rowptr[i + 1]; } else { b = e = 0; }
    };
    auto neighbour = [&](int b, int e) { return b + lane < e && lane < 64 ? g.col[b + lane] : 0; };
    auto source = [&](int c) { return g.n_id ? g.n_id[c] : (long long)c; };
    // prologue: fill the pipeline for the wave's first three rows
    rowptr_pair(wave, b0, e0);
    rowptr_pair(wave + nwaves, b1, e1);
    rowptr_pair(wave + 2 * nwaves, b2, e2);
    {
        const int c0 = neighbour(b0, e0);
        c1 = neighbour(b1, e1);
        id0 = source(c0);
        own0 = g.x_dst && wave < n_dst ? g.n_id[wave] : 0;
    }
    for (int i = wave; i < n_dst; i += nwaves) {
        // requests for the rows behind this one (nothing here depends on a load of this iteration)
        int b3, e3;
        rowptr_pair(i + 3 * nwaves, b3, e3);
        const int c2 = neighbour(b2, e2);
        const long long id1 = source(c1);
        const long long own1 = g.x_dst && i + nwaves < n_dst ? g.n_id[i + nwaves] : 0;
        // the data of row i
        const int beg = b0, end = e0, deg = end - beg;
        const float inv = deg > 0 ? 1.0f / (float)deg : 0.0f;
        for (int q0 = 0; q0 < C4; q0 += 192) {
            int q[3];
            bool ok[3];
            float4 s[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                q[k] = q0 + 64 * k + lane;
                ok[k] = q[k] < C4;
                s[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            for (int p = 0; p < deg; p += 4) {                             // four neighbour rows x three pieces in flight
                long long row[4];
                float w[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int pp = min(p + t, deg - 1);
                    w[t] = p + t < deg ? 1.0f : 0.0f;
                    if (deg <= 64) {
                        const int lo = __shfl((int)(unsigned)(id0 & 0xffffffffll), pp), hi = __shfl((int)(id0 >> 32), pp);
                        row[t] = ((long long)hi << 32) | (unsigned)lo;
                    } else {
                        row[t] = source(g.col[beg + pp]);                  // a long row: ids straight from memory
                    }
                }
                float4 v[4][3];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float4 *r = reinterpret_cast<const float4 *>(g.x + (size_t)row[t] * C);
#pragma unroll
                    for (int k = 0; k < 3; ++k) v[t][k] = r[ok[k] ? q[k] : 0];
                }
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        s[k].x += v[t][k].x * w[t]; s[k].y += v[t][k].y * w[t]; s[k].z += v[t][k].z * w[t]; s[k].w += v[t][k].w * w[t];
                    }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (!ok[k]) continue;
                s[k].x *= inv; s[k].y *= inv; s[k].z *= inv; s[k].w *= inv;
                reinterpret_cast<float4 *>(g.agg + (size_t)i * C)[q[k]] = s[k];
            }
            if (g.x_dst) {                                                 // the destination's own row: requested after the neighbour loop, so that
                const float4 *own = reinterpret_cast<const float4 *>(g.x + (size_t)own0 * C);      // it does not hold twelve registers across it
                float4 *dst = reinterpret_cast<float4 *>(g.x_dst + (size_t)i * C);
                const float4 o0 = own[ok[0] ? q[0] : 0], o1 = own[ok[1] ? q[1] : 0], o2 = own[ok[2] ? q[2] : 0];
                if (ok[0]) dst[q[0]] = o0;
                if (ok[1]) dst[q[1]] = o1;
                if (ok[2]) dst[q[2]] = o2;
            }
        }
        // advance the pipeline
        b0 = b1; e0 = e1; id0 = id1; own0 = own1;
        b1 = b2; e1 = e2; c1 = c2;
        b2 = b3; e2 = e3;
    }
}

// (registers are allotted per kernel, not per role: at the GEMM role's 138 a gather block's two extra waves per SIMD would not fit
//  beside a GEMM block -- 4 x 144 > 512 -- and the roles ran one after the other: 62 + 45 us.  Hence four waves per SIMD.)
template <int RB>
__global__ __launch_bounds__(T16_THREADS, 4) void k_gather_beside_gemm(T16Args a, GatherArgs g, int gemm_blocks) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if ((int)blockIdx.x < gemm_blocks) t16_block_loop<RB>(a, smem, (int)blockIdx.x, gemm_blocks);
    else gather_role(g, (int)blockIdx.x - gemm_blocks, (int)gridDim.x - gemm_blocks);
}

// (Round 4 built the layer as ONE launch -- the projection's tiles waiting, inside the launch, for their rows of the aggregate: 124-127 us
//  against 114-119 for these two launches; removed in round 5.)
template <int RB>
static int launch_gather_beside_gemm(const T16Args &a, const GatherArgs &g, int gemm_blocks, int gather_blocks, hipStream_t stream) {
    static LdsOptIn opt_in;
    if (!opt_in.done()) {
        POPE_HIP(hipFuncSetAttribute((const void *)k_gather_beside_gemm<RB>, hipFuncAttributeMaxDynamicSharedMemorySize, T16Shape<RB>::LDS_BYTES));
        opt_in.mark();
    }
    hipLaunchKernelGGL((k_gather_beside_gemm<RB>), dim3((unsigned)(gemm_blocks + gather_blocks)), dim3(T16_THREADS), T16Shape<RB>::LDS_BYTES, stream, a, g,
                       gemm_blocks);
    return POPE_OK;
}

// x: the matrix the rows are gathered from (the block's own sources, or the whole feature matrix with n_id); rb from
// forward_plan (3 .. 5).
static int forward_overlapped(const int32_t *rowptr, const int32_t *col, int64_t n_dst, const float *x, int32_t c_in, const long long *n_id,
                              float *x_dst, float *agg, const float *w_l, const float *b_l, const float *w_r, int32_t c_out, float *out,
                              const int32_t *dims, int rb, int cus, hipStream_t stream, BnStatsOut *stats) {
    T16Plan first, second;
    int rc;
    if ((rc = t16_fill(x, w_r, c_in, nullptr, nullptr, 0, c_in, c_in, (int)n_dst, c_out, b_l, out, c_out, dims, rb, cus, &first))) return rc;
    if ((rc = t16_fill(agg, w_l, c_in, nullptr, nullptr, 0, c_in, c_in, (int)n_dst, c_out, nullptr, out, c_out, dims, rb, cus, &second))) return rc;
    first.a.rows = n_id;                                            // nullptr: destination i is row i of x
    second.a.accumulate = 1;
    stats_take(stats, second);
    const int gemm_blocks = first.a.tiles_n == 2 ? std::min(first.grid, (cus + 15) / 16 * 16) : std::min(first.grid, cus);
    const int gather_blocks = cus;                                  // one per CU, beside its GEMM block (2-6 per CU measured: 2-10 us slower -- the row pipeline wants rows)
    const GatherArgs g{rowptr, col, (int)n_dst, x, c_in, agg, n_id, x_dst, dims};
    switch (rb) {
    case 3: rc = launch_gather_beside_gemm<3>(first.a, g, gemm_blocks, gather_blocks, stream); break;
    case 4: rc = launch_gather_beside_gemm<4>(first.a, g, gemm_blocks, gather_blocks, stream); break;
    default: rc = launch_gather_beside_gemm<5>(first.a, g, gemm_blocks, gather_blocks, stream); break;
    }
    if (rc) return rc;
    POPE_HIP(hipGetLastError());
    return t16_launch(second, stream);
}

// ---- both weight gradients as one stream-K launch (gemm_streamk_tn.h) ----
static bool streamk_tn_shape_ok(int64_t depth, int32_t M, int32_t Nb) {
    if ((M & 3) || (Nb & 3) || M < 4 || Nb < 4 || depth <= 0) return false;
    const long long tiles = 2ll * ((M + SK_TM - 1) / SK_TM) * ((Nb + SK_TN - 1) / SK_TN);
    return tiles * ((depth + SK_GK - 1) / SK_GK) >= 4ll * SK_MAX_GRID;
}

// One persistent block per CU (fewer if there are fewer units) for the twin of depth x M x Nb.
static int streamk_tn_grid(int cus, int64_t depth, int M, int Nb) {
    return streamk_grid(cus, 2ll * ((M + SK_TM - 1) / SK_TM) * ((Nb + SK_TN - 1) / SK_TN) * ((depth + SK_GK - 1) / SK_GK));
}

// C0 = G^T * B0, C1 = G^T * B1 (G [depth, M], B_q [depth, Nb], C_q [M, Nb]).  The caller has checked that the operands qualify
// (backward_plan: shape, alignment, a slab of sk_slab_bytes(grid)); grid and xcd are its choice.
static int gemm_streamk_tn(const float *G, const float *B0, const float *B1, int64_t depth, int M, int Nb, float *C0, float *C1,
                           void *slab, int grid, bool xcd, hipStream_t stream, const int *depth_dev, float *cs_part, float *cs_out,
                           const long long *rows1) {
    int rc;
    SkTnArgs a;
    a.G = G; a.ldg = M; a.B[0] = B0; a.B[1] = B1; a.ldb = Nb; a.C[0] = C0; a.C[1] = C1; a.ldc = Nb;
    a.M = M; a.Nb = Nb; a.depth = (int)depth; a.slab = (float *)slab;
    a.tiles_m = (M + SK_TM - 1) / SK_TM; a.tiles_nb = (Nb + SK_TN - 1) / SK_TN; a.S = (int)((depth + SK_GK - 1) / SK_GK);
    a.depth_dev = depth_dev;
    a.rows1 = rows1;
    // the bias gradient = column sums of G: its partial sums are a launch of their own in front of this one (BWD_COLSUM_PARTIAL: they
    // read G and nothing else), its final stage rides in the fix-up launch
    a.cs_part = cs_part; a.cs_out = cs_out; a.cs_splits = COLSUM_SPLITS; a.cs_C = M;
    const unsigned fix_blocks = 2u * a.tiles_m * a.tiles_nb + (cs_part ? (unsigned)(M + 15) / 16 : 0u);
    a.xcd = xcd;
    static LdsOptIn opt_in;
    if (!opt_in.done()) {
        POPE_HIP(hipFuncSetAttribute((const void *)k_gemm_streamk_tn<SK_GK>, hipFuncAttributeMaxDynamicSharedMemorySize, SkStage<SK_GK>::LDS_BYTES));
        opt_in.mark();
    }
    if ((rc = sk_zero_page(&a.zero))) return rc;
    hipLaunchKernelGGL(k_gemm_streamk_tn<SK_GK>, dim3((unsigned)grid), dim3(SKL_THREADS), SkStage<SK_GK>::LDS_BYTES, stream, a);
    hipLaunchKernelGGL(k_streamk_tn_fixup<SK_GK>, dim3(fix_blocks, SK_TN_FIX_PARTS), dim3(256), 0, stream, a, grid);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

// ---- which kernels a layer's backward pass runs, and in which order: decided HERE and nowhere else (no HIP calls) ----
// backward_plan writes the pass down as an ordered list of steps with their parameters.  conv_backward_impl walks the list and launches,
// sage_backward_kernel_name walks it and prints: one switch each, without a default, so a step that one of them forgets is a -Wall warning.
// Weight gradients (and, with them, the bias gradient), in this order of preference:
//   stream-K   BWD_COLSUM_PARTIAL (the bias gradient's partial sums: a launch in front), BWD_STREAMK (k_gemm_streamk_tn + k_streamk_tn_fixup
//              over one persistent block per CU, with the plain or the XCD-aware deal; the column sums' final stage in the fix-up launch)
//   dual       small layers with an input and a bias gradient: BWD_DUAL (k_gemm_dual: both twin GEMMs, the zeroing of grad_x's scatter-only
//              rows, the partial column sums), then BWD_SCATTER_AND_FINALS (the scatter and both reductions in one launch) -- the whole pass
//   twin       BWD_GATHER_ROWS (indexed mode only), BWD_W_TWIN (split-K k_gemm + k_slab_reduce for both weight gradients),
//              BWD_COLSUM_PARTIAL, BWD_COLSUM_FINAL
// and behind stream-K or twin, with an input gradient: BWD_ZERO_ROWS (n_src > n_dst), BWD_X_TWIN (the twin k_gemm of grad_x[:n_dst] and
// grad_agg), BWD_SCATTER_MEAN (a block with edges).
// Deterministic mode (g_sage_deterministic) changes the grad_x chain alone: no zeroing, no scatter (dual: BWD_FINALS, as without edges), and
// last BWD_DET_SUM: the index build and k_scatter_sum_det, which also writes the rows the scatter alone would have added to.
// Sum and max aggregation (`ordered`: sage_conv_backward_aggr) take that form of the chain whatever the mode, with BWD_ORDERED (the index
// build and aggregate.hip's k_scatter_ordered) in BWD_DET_SUM's place.
enum BwdStep : unsigned char {
    BWD_DUAL, BWD_SCATTER_AND_FINALS, BWD_FINALS, BWD_COLSUM_PARTIAL, BWD_STREAMK, BWD_GATHER_ROWS, BWD_W_TWIN, BWD_COLSUM_FINAL,
    BWD_ZERO_ROWS, BWD_X_TWIN, BWD_SCATTER_MEAN, BWD_DET_SUM, BWD_ORDERED
};
// 16-byte alignment of the operands: x = the matrix of the destination rows as the caller gave it (in indexed mode the feature
// matrix), x_tmp = the room for those rows as a matrix of their own (indexed mode, paths that cannot follow the index).
struct BwdAligned { bool grad_out, agg, x, x_tmp, w_l, w_r, grad_agg, grad_x, arg = true; };    // (arg: BWD_ORDERED under max)
struct BwdPlan {
    BwdStep steps[8];              // in launch order (the longest pass backward_plan can write: the twin path with every optional step, seven)
    int n_steps;
    void add(BwdStep s) { steps[n_steps++] = s; }
    int sk_grid;                   // BWD_STREAMK: persistent blocks,
    bool xcd;                      // ... dealt XCD-aware
    int splits;                    // BWD_DUAL, BWD_W_TWIN: depth splits of the weight-gradient twin
    GemmTile w_tile; GemmLayouts w_layouts;     // BWD_W_TWIN: tile and operand layouts
    bool colsum_vec;               // k_colsum_partial<true> (four columns per lane) or <false>, wherever it runs
    bool zero_rows;                // grad_x has rows that only the scatter adds to: BWD_ZERO_ROWS is a step, BWD_DUAL has zeroing blocks
    GemmTile x_tile; GemmLayouts x_layouts;     // BWD_X_TWIN: tile and operand layouts
    bool det_vec;                  // BWD_DET_SUM, BWD_ORDERED: k_scatter_sum_det<true> / k_scatter_ordered<OP, true> (16-byte accesses) or <false>
};

static BwdPlan backward_plan(int64_t n_dst, int64_t n_src, int32_t c_in, int32_t c_out, bool has_edges, bool need_grad_x, bool need_grad_b,
                             bool indexed, const BwdAligned &al, int cus, size_t slab_bytes, bool ordered = false) {
    BwdPlan p{};
    p.splits = weight_grad_splits(n_dst, c_in, c_out);
    p.colsum_vec = (c_out & 3) == 0 && al.grad_out;
    p.sk_grid = streamk_tn_grid(cus, n_dst, c_out, c_in);
    const bool streamk = streamk_tn_shape_ok(n_dst, c_out, c_in) && al.grad_out && al.agg && al.x && n_dst < INT32_MAX && slab_bytes >= sk_slab_bytes(p.sk_grid);
    if (streamk) {
        const int tiles_m = (c_out + SK_TM - 1) / SK_TM, tiles_nb = (c_in + SK_TN - 1) / SK_TN;
        const long long S = (n_dst + SK_GK - 1) / SK_GK;
        p.xcd = g_streamk_xcd && p.sk_grid % 8 == 0 && (p.sk_grid / 8) % tiles_m == 0 && p.sk_grid / tiles_m <= 2ll * tiles_nb * S;
    }
    const bool gather_rows = !streamk && indexed;                 // the other kernels want the destination rows as a matrix
    const bool x_al = gather_rows ? al.x_tmp : al.x;
    const int M = (int)n_dst;
    // operands as conv_backward_impl builds them: (outer, depth) strides
    const Layout g = pick_layout(al.grad_out, c_out, 1, M, c_out), gt = pick_layout(al.grad_out, 1, c_out, c_out, M);
    const Layout wr_t = pick_layout(al.w_r, 1, c_in, c_in, c_out), wl_t = pick_layout(al.w_l, 1, c_in, c_in, c_out);
    const Layout agg_t = pick_layout(al.agg, 1, c_in, c_in, M), xd_t = pick_layout(x_al, 1, c_in, c_in, M);
    // dual: both twins would take 64 x 64 tiles
    const bool dual = !streamk && need_grad_x && p.splits > 1 && need_grad_b && p.colsum_vec && g == LAYOUT_KC_VEC && wr_t == LAYOUT_OC_VEC &&
                      wl_t == LAYOUT_OC_VEC && gt == LAYOUT_OC_VEC && agg_t == LAYOUT_OC_VEC && xd_t == LAYOUT_OC_VEC &&
                      tiles(M, c_in, 64, 128) * 2 < 384 && tiles(c_out, c_in, 64, 128) * p.splits * 2 < 384;
    const bool det_sum = (g_sage_deterministic || ordered) && need_grad_x;
    const bool scatter = need_grad_x && has_edges && !det_sum;
    p.zero_rows = need_grad_x && n_src > n_dst && !det_sum;
    p.det_vec = (c_in & 3) == 0 && al.grad_agg && al.grad_x && al.arg;
    if (dual) {
        p.add(BWD_DUAL);
        p.add(scatter ? BWD_SCATTER_AND_FINALS : BWD_FINALS);
        if (det_sum) p.add(ordered ? BWD_ORDERED : BWD_DET_SUM);
        return p;
    }
    if (streamk) {
        if (need_grad_b) p.add(BWD_COLSUM_PARTIAL);
        p.add(BWD_STREAMK);
    } else {
        if (gather_rows) p.add(BWD_GATHER_ROWS);
        p.w_tile = gemm_tile_for(c_out, c_in, p.splits, 2);
        p.w_layouts = gemm_layouts(gt, agg_t, false, LAYOUT_GENERIC, LAYOUT_GENERIC, true, xd_t);
        p.add(BWD_W_TWIN);
        if (need_grad_b) {
            p.add(BWD_COLSUM_PARTIAL);
            p.add(BWD_COLSUM_FINAL);
        }
    }
    if (need_grad_x) {
        if (p.zero_rows) p.add(BWD_ZERO_ROWS);
        p.x_tile = gemm_tile_for(M, c_in, 1, 2);
        p.x_layouts = gemm_layouts(g, wr_t, false, LAYOUT_GENERIC, LAYOUT_GENERIC, true, wl_t);
        p.add(BWD_X_TWIN);
        if (scatter) p.add(BWD_SCATTER_MEAN);
        if (det_sum) p.add(ordered ? BWD_ORDERED : BWD_DET_SUM);
    }
    return p;
}

}  // namespace pope

using namespace pope;

#ifdef POPE_STAMP
extern "C" int pope_debug_read_t16_trace(unsigned long long *host, int count) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_t16_trace), (size_t)count * sizeof(unsigned long long));
}
extern "C" int pope_debug_read_gemm_stamps(unsigned long long *host, int count) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_gemm_stamps), (size_t)count * sizeof(unsigned long long));
}
#endif

// dst[i, :] = x[rows[i], :], i < n (a device extent may shorten n): the destination rows of a sampled block as a matrix of
// their own, for the kernel paths that cannot read them through n_id.
__global__ __launch_bounds__(256) void k_gather_rows(const float *__restrict__ x, const long long *__restrict__ rows, int n, int C,
                                                     float *__restrict__ dst, const int *__restrict__ n_dev) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    n = dyn_extent(n_dev, n);
    for (int i = wave; i < n; i += nwaves) {
        const float *src = x + (size_t)rows[i] * C;
        float *d = dst + (size_t)i * C;
        if ((C & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
            for (int q = lane; q < (C >> 2); q += 64) reinterpret_cast<float4 *>(d)[q] = reinterpret_cast<const float4 *>(src)[q];
        } else {
            for (int c = lane; c < C; c += 64) d[c] = src[c];
        }
    }
}

static size_t rows_matrix_bytes(int64_t n_dst, int32_t c_in) { return align_up((size_t)n_dst * c_in * sizeof(float), 256); }

// ---- where everything lies in the scratch buffer of the backward pass: laid out HERE and nowhere else ----
// Byte offsets, each a multiple of 256, a function of the sizes alone (never of the length of the buffer the caller passed):
//   core     grad_agg [n_dst, c_in] | split-K / stream-K slabs of the two weight gradients (one twin launch) | the partial column sums of
//            the bias gradient (a region of its own: they are computed beside the weight gradients); nothing for a layer without rows or columns
//   index    of the deterministic sum, if asked for and the block's sizes are valid: start [n_src + 1] | list [nnz] | sorted [nnz], int32 each
//   rows     indexed mode: the destination rows as a matrix [n_dst, c_in], for the kernel paths that cannot follow the index
// sage_scatter_mean_det on its own is the layer without columns: the index at offset 0.
struct BwdScratch {
    size_t grad_agg, slab, slab_bytes, colsum, core;             // (core: the bytes of the three core regions together)
    size_t det_start, det_list, det_sorted, rows, total;
};

static BwdScratch backward_scratch(int64_t n_src, int64_t n_dst, int64_t nnz, int32_t c_in, int32_t c_out, bool deterministic, bool indexed) {
    BwdScratch s{};
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t was = at; at += align_up(bytes, 256); return was; };
    if (n_dst > 0 && c_in > 0 && c_out > 0) {
        s.grad_agg = take((size_t)n_dst * c_in * sizeof(float));
        s.slab_bytes = 2 * (size_t)weight_grad_splits(n_dst, c_in, c_out) * c_out * c_in * sizeof(float);
        if (streamk_tn_shape_ok(n_dst, c_out, c_in) && s.slab_bytes < sk_slab_bytes(SK_MAX_GRID)) s.slab_bytes = sk_slab_bytes(SK_MAX_GRID);
        s.slab_bytes = align_up(s.slab_bytes, 256);
        s.slab = take(s.slab_bytes);
        s.colsum = take((size_t)COLSUM_SPLITS * c_out * sizeof(float));
        s.core = at;
    }
    if (deterministic && n_src > 0 && n_dst >= 0 && n_dst <= n_src && nnz >= 0 && n_src < INT32_MAX && nnz < INT32_MAX) {
        s.det_start = take((size_t)(n_src + 1) * sizeof(int));
        s.det_list = take((size_t)(nnz > 0 ? nnz : 1) * sizeof(int));
        s.det_sorted = take((size_t)(nnz > 0 ? nnz : 1) * sizeof(int));
    }
    if (indexed && s.core) s.rows = take(rows_matrix_bytes(n_dst, c_in));
    s.total = at;
    return s;
}

template <typename T>
static T *scratch_at(void *scratch, size_t offset) { return reinterpret_cast<T *>(static_cast<char *>(scratch) + offset); }

// ---- the name buffer, the launch sinks and the host parts the whole-graph layers share, included in place ----
#include "layer_host.h"

extern "C" size_t sage_scatter_mean_det_scratch_bytes(int64_t n_src, int64_t n_dst, int64_t nnz) {
    return backward_scratch(n_src, n_dst, nnz, 0, 0, true, false).total;
}

extern "C" int32_t sage_set_deterministic(int32_t on) {
    const int32_t was = g_sage_deterministic;
    g_sage_deterministic = on != 0;
    return was;
}

extern "C" int32_t sage_get_deterministic(void) { return g_sage_deterministic; }

// (a layer without rows or columns has no backward pass: 0, whatever the mode)
extern "C" size_t sage_conv_scratch_bytes(int64_t n_src, int64_t n_dst, int64_t nnz, int32_t c_in, int32_t c_out) {
    const BwdScratch s = backward_scratch(n_src, n_dst, nnz, c_in, c_out, g_sage_deterministic, false);
    return s.core ? s.total : 0;
}

extern "C" size_t sage_conv_forward_scratch_bytes(int64_t n_dst, int32_t c_in, int32_t c_out) {
    if (n_dst <= 0 || c_in <= 0 || c_out <= 0) return 0;
    return streamk_shape_ok(n_dst, c_in, c_in, c_out) ? sk_slab_bytes(SK_MAX_GRID) : 0;
}

// The indexed entry points may be called without an x_dst matrix (the destination rows are then read through n_id); the
// kernel paths that cannot do that build the matrix in the tail of the scratch buffer.
extern "C" size_t sage_conv_forward_indexed_scratch_bytes(int64_t n_dst, int32_t c_in, int32_t c_out) {
    if (n_dst <= 0 || c_in <= 0 || c_out <= 0) return 0;
    return align_up(sage_conv_forward_scratch_bytes(n_dst, c_in, c_out), 256) + rows_matrix_bytes(n_dst, c_in);
}

extern "C" size_t sage_conv_backward_indexed_scratch_bytes(int64_t n_src, int64_t n_dst, int64_t nnz, int32_t c_in, int32_t c_out) {
    const BwdScratch s = backward_scratch(n_src, n_dst, nnz, c_in, c_out, g_sage_deterministic, true);
    return s.core ? s.total : 0;
}

// vec: c_in % 4 == 0 and x_src, agg and x_dst (if any) are 16-byte aligned
static void enqueue_gather_mean(const int32_t *rowptr, const int32_t *col, int64_t n_dst, const float *x_src, int32_t c_in,
                                float *agg, bool vec, hipStream_t stream, const int64_t *n_id = nullptr, float *x_dst = nullptr,
                                const int32_t *n_dst_dev = nullptr) {
    dim3 grid(capped_grid((size_t)n_dst * 64, 256));
    if (vec)
        hipLaunchKernelGGL(k_gather_mean<true>, grid, dim3(256), 0, stream, rowptr, col, (int)n_dst, x_src, c_in, agg,
                           (const long long *)n_id, x_dst, n_dst_dev);
    else
        hipLaunchKernelGGL(k_gather_mean<false>, grid, dim3(256), 0, stream, rowptr, col, (int)n_dst, x_src, c_in, agg,
                           (const long long *)n_id, x_dst, n_dst_dev);
}

extern "C" int sage_gather_mean(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz,
                                const float *x_src, int32_t c_in, float *agg, void *stream_) {
    clear_error();
    POPE_REQUIRE(rowptr && (col || nnz == 0) && x_src && agg, "sage_gather_mean: null pointer");
    POPE_REQUIRE(n_dst > 0 && n_src > 0 && n_src < INT32_MAX && nnz >= 0 && nnz < INT32_MAX && c_in > 0, "sage_gather_mean: bad size");
    enqueue_gather_mean(rowptr, col, n_dst, x_src, c_in, agg, (c_in & 3) == 0 && aligned16(x_src) && aligned16(agg), (hipStream_t)stream_);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

// The layer after validation: plan, then launch per plan.  x [x_rows, c_in] is the matrix the rows are gathered from: the
// block's own sources (n_id == nullptr; the destinations are its first n_dst rows), or the resident feature matrix read
// through n_id, with x_dst the matrix of the destination rows (written here; nullptr: kept in the tail of the scratch
// buffer by the paths that need it).
static int conv_forward_run(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_dst, const float *x, int64_t x_rows,
                            int32_t c_in, const float *w_l, const float *b_l, const float *w_r, int32_t c_out, float *agg, float *x_dst,
                            float *out, void *scratch, size_t scratch_bytes, const int32_t *dims, BnStatsOut *stats, hipStream_t stream) {
    int cus = 0, rc;
    if ((rc = device_cu_count(&cus))) return rc;
    const size_t rows_at = align_up(sage_conv_forward_scratch_bytes(n_dst, c_in, c_out), 256);   // the destination rows' place in the scratch buffer
    float *const x_dst_tail = scratch ? (float *)((char *)scratch + rows_at) : nullptr;
    const float *own = !n_id ? x : x_dst ? x_dst : x_dst_tail;
    const FwdAligned al{aligned16(x), aligned16(agg), aligned16(own), !x_dst || aligned16(x_dst), aligned16(w_l), aligned16(w_r)};
    const FwdPlan plan = forward_plan(n_dst, c_in, c_out, x_rows, cus, al, !scratch ? 0 : n_id && !x_dst ? rows_at : scratch_bytes);
    if (plan.path == FWD_OVERLAPPED)
        return forward_overlapped(rowptr, col, n_dst, x, c_in, (const long long *)n_id, x_dst, agg, w_l, b_l, w_r, c_out, out, dims, plan.rb, cus,
                                  stream, stats);
    if (n_id && !x_dst) {                                            // no matrix of the destination rows from the caller: the kernels below want one
        if (!scratch || scratch_bytes < rows_at + rows_matrix_bytes(n_dst, c_in)) {
            set_error("sage_conv_forward_indexed: without x_dst the scratch must hold sage_conv_forward_indexed_scratch_bytes (%zu), got %zu",
                      rows_at + rows_matrix_bytes(n_dst, c_in), scratch_bytes);
            return POPE_ERR_WORKSPACE;
        }
        x_dst = x_dst_tail;
    }
    enqueue_gather_mean(rowptr, col, n_dst, x, c_in, agg, plan.gather_vec, stream, n_id, x_dst, dims);
    // out = agg * w_l^T + b_l + x_dst * w_r^T in one pass
    switch (plan.path) {
    case FWD_TILE16:
        return gemm_tile16(agg, w_l, c_in, own, w_r, c_in, c_in, c_in, (int)n_dst, c_out, b_l, out, c_out, plan.rb, cus, stream, dims, stats);
    case FWD_STREAMK:
        return gemm_streamk(agg, w_l, c_in, own, w_r, c_in, c_in, c_in, (int)n_dst, c_out, b_l, out, c_out, scratch, cus, stream, dims);
    default: {
        GemmArgs p = gemm_problem(Operand{agg, c_in, 1}, Operand{w_l, c_in, 1}, c_in, (int)n_dst, c_out, out, c_out);
        p.A1 = Operand{own, c_in, 1}; p.B1 = Operand{w_r, c_in, 1}; p.K1 = c_in;
        p.bias = b_l;
        p.m_dev = dims;
        return launch_gemm(p, plan.tile, plan.layouts, stream);
    }
    }
}

// `dims` (device int32 [4] = {n_dst, n_src, nnz, 0}, or NULL): see include/graphpope_hip.h, "Device extents".
static int conv_forward_impl(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz,
                             const float *x_src, int32_t c_in, const float *w_l, const float *b_l, const float *w_r,
                             int32_t c_out, float *agg, float *out, void *scratch, size_t scratch_bytes, const int32_t *dims,
                             BnStatsOut *stats, hipStream_t stream) {
    POPE_REQUIRE(rowptr && (col || nnz == 0) && x_src && w_l && w_r && agg && out, "sage_conv_forward: null pointer");
    POPE_REQUIRE(n_dst > 0 && n_dst <= n_src && n_src < INT32_MAX && nnz >= 0 && nnz < INT32_MAX && c_in > 0 && c_out > 0,
                 "sage_conv_forward: bad size (destinations must be the first n_dst sources)");
    return conv_forward_run(rowptr, col, nullptr, n_dst, x_src, n_src, c_in, w_l, b_l, w_r, c_out, agg, nullptr, out, scratch, scratch_bytes, dims,
                            stats, stream);
}

// The same layer on rows of the resident feature matrix: source j of the block is feats[n_id[j]].  Replaces
// Batch.x = data.x[n_id] (main.py:118-123) + the layer: x[n_id] is never materialised, only the n_dst destination rows
// (x_dst, needed again by the backward pass) are.
static int conv_forward_indexed_impl(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst,
                                     int64_t nnz, const float *feats, int64_t n_rows, int32_t c_in, const float *w_l,
                                     const float *b_l, const float *w_r, int32_t c_out, float *agg, float *x_dst, float *out,
                                     void *scratch, size_t scratch_bytes, const int32_t *dims, BnStatsOut *stats, hipStream_t stream) {
    POPE_REQUIRE(rowptr && (col || nnz == 0) && n_id && feats && w_l && w_r && agg && out, "sage_conv_forward_indexed: null pointer");
    POPE_REQUIRE(n_dst > 0 && n_dst <= n_src && n_src < INT32_MAX && n_rows > 0 && nnz >= 0 && nnz < INT32_MAX && c_in > 0 && c_out > 0,
                 "sage_conv_forward_indexed: bad size (destinations must be the first n_dst entries of n_id)");
    return conv_forward_run(rowptr, col, n_id, n_dst, feats, n_rows, c_in, w_l, b_l, w_r, c_out, agg, x_dst, out, scratch, scratch_bytes, dims,
                            stats, stream);
}

// The kernels sage_conv_forward(_indexed)(_stats) launches for a layer of this shape on a device of cu_count CUs, as a kernel
// trace shows them: forward_plan with host extents and the scratch the size queries ask for.  Bit i of `misaligned`: field i of
// FwdAligned is not 16-byte aligned.  With a mask the gather kernel is named in front of the projection (the overlapped form
// carries it) and the plain tile kernel with all six template arguments, the operand layouts last.
extern "C" int sage_forward_kernel_name_at(int64_t n_dst, int32_t c_in, int32_t c_out, int32_t cu_count, uint32_t misaligned, char *name,
                                           size_t cap) {
    clear_error();
    POPE_REQUIRE(name && cap > 0 && n_dst > 0 && n_dst < INT32_MAX && c_in > 0 && c_out > 0 && cu_count > 0 && misaligned < (1u << 6),
                 "sage_forward_kernel_name: bad argument");
    const auto ok = [misaligned](int bit) { return !(misaligned >> bit & 1u); };
    const FwdPlan p = forward_plan(n_dst, c_in, c_out, n_dst, cu_count, FwdAligned{ok(0), ok(1), ok(2), ok(3), ok(4), ok(5)},
                                   sage_conv_forward_scratch_bytes(n_dst, c_in, c_out));
    char gather[32] = "";
    if (misaligned && p.path != FWD_OVERLAPPED) snprintf(gather, sizeof gather, "k_gather_mean<%s>+", p.gather_vec ? "true" : "false");
    switch (p.path) {
    case FWD_OVERLAPPED: snprintf(name, cap, "k_gather_beside_gemm<%d>+k_gemm_tile16<%d, %d>", p.rb, p.rb, t16_buffers()); break;
    case FWD_TILE16:     snprintf(name, cap, "%sk_gemm_tile16<%d, %d>", gather, p.rb, t16_buffers()); break;
    case FWD_STREAMK:    snprintf(name, cap, "%sk_gemm_streamk_ld<%d>", gather, SK_GK); break;
    default:
        if (misaligned)
            snprintf(name, cap, "%sk_gemm<%d, %d, %d, %d, %d, %d>", gather, p.tile.tm, p.tile.tn, p.tile.tm == 128 ? 4 : 2, p.tile.tm == 128 ? 1 : 2,
                     (int)p.layouts.a, (int)p.layouts.b);
        else snprintf(name, cap, "k_gemm<%d, %d>", p.tile.tm, p.tile.tn);
        break;
    }
    return POPE_OK;
}

extern "C" int sage_forward_kernel_name(int64_t n_dst, int32_t c_in, int32_t c_out, int32_t cu_count, char *name, size_t cap) {
    return sage_forward_kernel_name_at(n_dst, c_in, c_out, cu_count, 0, name, cap);
}

extern "C" int sage_conv_forward(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz,
                                 const float *x_src, int32_t c_in, const float *w_l, const float *b_l, const float *w_r,
                                 int32_t c_out, float *agg, float *out, void *scratch, size_t scratch_bytes, const int32_t *dims,
                                 void *stream_) {
    clear_error();
    return conv_forward_impl(rowptr, col, n_src, n_dst, nnz, x_src, c_in, w_l, b_l, w_r, c_out, agg, out, scratch, scratch_bytes, dims, nullptr,
                             (hipStream_t)stream_);
}

extern "C" int sage_conv_forward_indexed(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst,
                                         int64_t nnz, const float *feats, int64_t n_rows, int32_t c_in, const float *w_l,
                                         const float *b_l, const float *w_r, int32_t c_out, float *agg, float *x_dst, float *out,
                                         void *scratch, size_t scratch_bytes, const int32_t *dims, void *stream_) {
    clear_error();
    return conv_forward_indexed_impl(rowptr, col, n_id, n_src, n_dst, nnz, feats, n_rows, c_in, w_l, b_l, w_r, c_out, agg, x_dst, out, scratch,
                                     scratch_bytes, dims, nullptr, (hipStream_t)stream_);
}

// The same two calls for a layer whose output goes into BatchNorm (main.py:206-207: x = convs[i](...); x = bns[i](x)): the projection's
// epilogue also leaves the column sums of `out` and of its squares per row tile in bn_pa / bn_pb ([bn_parts_cap, c_out] doubles each;
// bn_parts_cap >= ceil(n_dst / 16) always suffices) -- the first stage of the BatchNorm statistics, which was a launch of its own
// re-reading `out`.  bn_info[0] = row tiles written, bn_info[1] = rows per tile (host ints); bn_info[0] = 0: this shape's kernel
// path produces no statistics, run sage_bn_relu_dropout_forward; else sage_bn_relu_dropout_forward_stats.
extern "C" int sage_conv_forward_stats(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz,
                                       const float *x_src, int32_t c_in, const float *w_l, const float *b_l, const float *w_r,
                                       int32_t c_out, float *agg, float *out, void *scratch, size_t scratch_bytes, const int32_t *dims,
                                       double *bn_pa, double *bn_pb, int32_t bn_parts_cap, int32_t *bn_info, void *stream_) {
    clear_error();
    POPE_REQUIRE(bn_pa && bn_pb && bn_info && bn_parts_cap > 0, "sage_conv_forward_stats: null pointer");
    BnStatsOut st{bn_pa, bn_pb, bn_parts_cap};
    return stats_report(conv_forward_impl(rowptr, col, n_src, n_dst, nnz, x_src, c_in, w_l, b_l, w_r, c_out, agg, out, scratch, scratch_bytes, dims, &st,
                                          (hipStream_t)stream_), st, bn_info);
}

extern "C" int sage_conv_forward_indexed_stats(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst,
                                               int64_t nnz, const float *feats, int64_t n_rows, int32_t c_in, const float *w_l,
                                               const float *b_l, const float *w_r, int32_t c_out, float *agg, float *x_dst, float *out,
                                               void *scratch, size_t scratch_bytes, const int32_t *dims, double *bn_pa, double *bn_pb,
                                               int32_t bn_parts_cap, int32_t *bn_info, void *stream_) {
    clear_error();
    POPE_REQUIRE(bn_pa && bn_pb && bn_info && bn_parts_cap > 0, "sage_conv_forward_indexed_stats: null pointer");
    BnStatsOut st{bn_pa, bn_pb, bn_parts_cap};
    return stats_report(conv_forward_indexed_impl(rowptr, col, n_id, n_src, n_dst, nnz, feats, n_rows, c_in, w_l, b_l, w_r, c_out, agg, x_dst, out,
                                                  scratch, scratch_bytes, dims, &st, (hipStream_t)stream_), st, bn_info);
}

// The deterministic sum behind validation: the index build (skipped for a block without room for an edge) and the sum kernel,
// vectorised (`vec`) if c % 4 == 0 and gagg and grad_x are 16-byte aligned.  The index lies in `scratch` where `lay` says.
void pope::enqueue_det_block_index(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, int *start, int *list,
                                   const int32_t *dims, hipStream_t stream) {
    const int32_t *n_dst_dev = dims, *n_src_dev = dims ? dims + 1 : nullptr;
    hipLaunchKernelGGL(k_det_clear, dim3(capped_grid((size_t)n_src + 1, 256)), dim3(256), 0, stream, start, (int)n_src, n_src_dev);
    if (nnz > 0 && n_dst > 0) {
        const dim3 rows(capped_grid((size_t)n_dst * 64, 256));
        hipLaunchKernelGGL(k_det_index<false>, rows, dim3(256), 0, stream, rowptr, col, (int)n_dst, (int)n_src, (int)nnz, start, list, n_dst_dev, n_src_dev);
        hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(DET_SCAN_THREADS), 0, stream, start, (int)n_src, n_src_dev);
        hipLaunchKernelGGL(k_det_index<true>, rows, dim3(256), 0, stream, rowptr, col, (int)n_dst, (int)n_src, (int)nnz, start, list, n_dst_dev, n_src_dev);
    }
}

static void enqueue_scatter_sum_det(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, const float *gagg,
                                    int32_t c, float *grad_x, bool vec, void *scratch, const BwdScratch &lay, const int32_t *dims,
                                    hipStream_t stream) {
    int *start = scratch_at<int>(scratch, lay.det_start), *list = scratch_at<int>(scratch, lay.det_list);
    int *sorted = scratch_at<int>(scratch, lay.det_sorted);
    const int32_t *n_dst_dev = dims, *n_src_dev = dims ? dims + 1 : nullptr;
    enqueue_det_block_index(rowptr, col, n_src, n_dst, nnz, start, list, dims, stream);
    const dim3 grid(capped_grid((size_t)n_src * ((c + 255) / 256) * 64, 256));
    if (vec)
        hipLaunchKernelGGL(k_scatter_sum_det<true>, grid, dim3(256), 0, stream, rowptr, start, list, sorted, (int)n_dst, (int)n_src, (int)nnz, gagg, c,
                           grad_x, n_dst_dev, n_src_dev);
    else
        hipLaunchKernelGGL(k_scatter_sum_det<false>, grid, dim3(256), 0, stream, rowptr, start, list, sorted, (int)n_dst, (int)n_src, (int)nnz, gagg, c,
                           grad_x, n_dst_dev, n_src_dev);
}

// Its sibling for sum and max aggregation: the same index, then k_scatter_ordered (aggregate.hip).
static void enqueue_ordered_sum(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, const int32_t *arg,
                                const float *gagg, int32_t c, int aggr, float *grad_x, bool vec, void *scratch, const BwdScratch &lay,
                                const int32_t *dims, hipStream_t stream) {
    int *start = scratch_at<int>(scratch, lay.det_start), *list = scratch_at<int>(scratch, lay.det_list);
    enqueue_det_block_index(rowptr, col, n_src, n_dst, nnz, start, list, dims, stream);
    enqueue_scatter_ordered(rowptr, n_src, n_dst, nnz, start, list, scratch_at<int>(scratch, lay.det_sorted), arg, gagg, c, aggr, grad_x, vec, dims,
                            stream);
}

// The scatter of the backward pass as a sum in a fixed order (include/graphpope_hip.h: the contract).
extern "C" int sage_scatter_mean_det(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, const float *grad_agg,
                                     int32_t c, float *grad_x, void *scratch, size_t scratch_bytes, const int32_t *dims, void *stream_) {
    clear_error();
    POPE_REQUIRE(n_src >= 0 && n_dst >= 0 && n_dst <= n_src && n_src < INT32_MAX && nnz >= 0 && nnz < INT32_MAX && c > 0,
                 "sage_scatter_mean_det: bad size (destinations must be the first n_dst sources)");
    if (n_src == 0) return POPE_OK;
    POPE_REQUIRE(rowptr && (col || nnz == 0) && grad_agg && grad_x && scratch, "sage_scatter_mean_det: null pointer");
    const BwdScratch lay = backward_scratch(n_src, n_dst, nnz, 0, 0, true, false);
    POPE_REQUIRE(scratch_bytes >= lay.total, "sage_scatter_mean_det: scratch %zu < %zu bytes", scratch_bytes, lay.total);
    if (nnz == 0 && n_src == n_dst) return POPE_OK;                 // nothing to add and no row behind the destinations to overwrite
    enqueue_scatter_sum_det(rowptr, col, n_src, n_dst, nnz, grad_agg, c, grad_x, (c & 3) == 0 && aligned16(grad_agg) && aligned16(grad_x), scratch,
                            lay, dims, (hipStream_t)stream_);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

// Small layer (the weight gradients did not qualify for the stream-K kernel) with an input gradient: the two twin GEMMs (px: grad_x and
// grad_agg, pw: the weight gradients' slabs), the zeroing of grad_x's scatter-only rows and the bias gradient's partial sums all read
// grad_out and nothing of one another -- one launch of 64 x 64 tiles.
static int launch_gemm_dual(GemmArgs px, GemmArgs pw, const DualAux &aux, hipStream_t stream) {
    gemm_set_grid(px, 64, 64);
    gemm_set_grid(pw, 64, 64);
    const size_t lds = tile_lds_bytes<64, 64>();
    static LdsOptIn opt_in;
    if (!opt_in.done()) {
        POPE_HIP(hipFuncSetAttribute((const void *)k_gemm_dual<64, 64, 2, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        opt_in.mark();
    }
    const int blocks = px.gx * px.gy * px.gz + pw.gx * pw.gy * pw.gz + aux.zero_blocks + aux.cs_gx * aux.cs_gy;
    hipLaunchKernelGGL((k_gemm_dual<64, 64, 2, 2>), dim3(blocks), dim3(256), lds, stream, px, pw, aux);
    return POPE_OK;
}

// (Round 3 measured the bias gradient and the grad_x chain on side streams beside the weight gradients: 0.449 ms against 0.378 ms on
//  one stream -- every fork / join is two cross-stream dependencies and a side kernel on a CU delays the statically dealt stream-K
//  launch; removed in round 5.)
// x_rows == nullptr: x_src holds the block's source rows (the destinations first).  Otherwise the destination rows are
// x_src[x_rows[i]] (the resident feature matrix read through n_id), and the kernel paths that cannot follow the index build them
// as a matrix in the scratch buffer.  `lay`: the layout of `scratch` for these sizes, which the caller has checked the buffer against.
static int conv_backward_impl(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, const float *x_src,
                              const long long *x_rows, const float *agg, int32_t c_in, const float *w_l, const float *w_r, int32_t c_out,
                              const float *grad_out, float *grad_x, float *grad_w_l, float *grad_b_l, float *grad_w_r, void *scratch,
                              const BwdScratch &lay, const int32_t *dims, hipStream_t stream, int aggr = POPE_AGGR_MEAN,
                              const int32_t *arg = nullptr) {
    float *const gagg = scratch_at<float>(scratch, lay.grad_agg), *const slab = scratch_at<float>(scratch, lay.slab);
    float *const colsum = scratch_at<float>(scratch, lay.colsum), *const x_tmp = x_rows ? scratch_at<float>(scratch, lay.rows) : nullptr;
    const int32_t *n_dst_dev = dims, *n_src_dev = dims ? dims + 1 : nullptr;
    int cus = 0, rc = POPE_OK;
    if (streamk_tn_shape_ok(n_dst, c_out, c_in) && (rc = device_cu_count(&cus))) return rc;   // (only the stream-K grid depends on it)
    const BwdAligned al{aligned16(grad_out), aligned16(agg), aligned16(x_src), aligned16(x_tmp), aligned16(w_l), aligned16(w_r), aligned16(gagg),
                        aligned16(grad_x), aligned16(arg)};
    const BwdPlan plan = backward_plan(n_dst, n_src, c_in, c_out, nnz > 0, grad_x != nullptr, grad_b_l != nullptr, x_rows != nullptr, al, cus,
                                       lay.slab_bytes, aggr != POPE_AGGR_MEAN);

    // The two twin products of the plain tile kernel (BWD_DUAL runs both, BWD_W_TWIN and BWD_X_TWIN one each).  Operands as (outer, depth):
    // grad_w_l[o, c] = sum_i grad_out[i, o] * agg[i, c], grad_w_r likewise with the destination rows (BWD_GATHER_ROWS: x_tmp): depth = rows i, split
    GemmArgs pw = gemm_problem(Operand{grad_out, 1, c_out}, Operand{agg, 1, c_in}, (int)n_dst, c_out, c_in, grad_w_l, c_in);
    pw.twin.B = Operand{x_src, 1, c_in}; pw.twin.C = grad_w_r; pw.gz = plan.splits; pw.slab = slab; pw.k0_dev = n_dst_dev;
    // grad_x[:n_dst] = grad_out * w_r and grad_agg = grad_out * w_l (w^T: outer c, depth o), which the scatter or the deterministic sum adds to grad_x
    GemmArgs px = gemm_problem(Operand{grad_out, c_out, 1}, Operand{w_r, 1, c_in}, c_out, (int)n_dst, c_in, grad_x, c_in);
    px.twin.B = Operand{w_l, 1, c_in}; px.twin.C = gagg; px.m_dev = n_dst_dev;
    // both reductions behind BWD_DUAL: the weight gradients' slabs, then the bias gradient's partial sums
    const int reduce_blocks = (int)capped_grid((size_t)c_out * c_in * 2, 256), finals_blocks = reduce_blocks + (c_out + 15) / 16;
    const BwdFinals fin{slab, plan.splits, (size_t)c_out * c_in, c_in, grad_w_l, grad_w_r, (long long)c_in, reduce_blocks, colsum, COLSUM_SPLITS, c_out, grad_b_l};
    const dim3 scatter_grid(capped_grid((size_t)n_dst * ((c_in + 255) / 256) * 64, 256));

    for (int s = 0; s < plan.n_steps && !rc; ++s) {
        switch (plan.steps[s]) {
        case BWD_DUAL: {
            DualAux aux;
            aux.zero_x = plan.zero_rows ? grad_x : nullptr;
            aux.zero_C = c_in; aux.zero_r0 = (int)n_dst; aux.zero_r1 = (int)n_src; aux.zero_r0_dev = n_dst_dev; aux.zero_r1_dev = n_src_dev;
            aux.zero_blocks = aux.zero_x ? (int)capped_grid((size_t)n_src * c_in / 4 / 8 + 1, 256, 256) : 0;
            aux.cs_g = grad_out; aux.cs_rows = (int)n_dst; aux.cs_C = c_out; aux.cs_part = colsum; aux.cs_rows_dev = n_dst_dev;
            const dim3 cs = colsum_partial_grid(c_out, true);       // (backward_plan: dual only with colsum_vec)
            aux.cs_gx = (int)cs.x; aux.cs_gy = (int)cs.y;
            rc = launch_gemm_dual(px, pw, aux, stream);
            break;
        }
        case BWD_SCATTER_AND_FINALS:
            hipLaunchKernelGGL(k_scatter_and_finals, dim3(finals_blocks + scatter_grid.x), dim3(256), 0, stream, rowptr, col, (int)n_dst, gagg, c_in,
                               grad_x, n_dst_dev, fin, finals_blocks);
            break;
        case BWD_FINALS:         hipLaunchKernelGGL(k_bwd_finals, dim3(finals_blocks), dim3(256), 0, stream, fin); break;
        case BWD_COLSUM_PARTIAL: enqueue_colsum_partial(grad_out, (int)n_dst, c_out, colsum, n_dst_dev, plan.colsum_vec, stream); break;
        case BWD_STREAMK:                                       // (reads the destination rows through x_rows, if there is an index)
            rc = gemm_streamk_tn(grad_out, agg, x_src, n_dst, c_out, c_in, grad_w_l, grad_w_r, slab, plan.sk_grid, plan.xcd, stream, n_dst_dev,
                                 grad_b_l ? colsum : nullptr, grad_b_l, x_rows);
            break;
        case BWD_GATHER_ROWS:
            hipLaunchKernelGGL(k_gather_rows, dim3(capped_grid((size_t)n_dst * 64, 256)), dim3(256), 0, stream, x_src, x_rows, (int)n_dst, c_in, x_tmp,
                               n_dst_dev);
            pw.twin.B.p = x_tmp;
            break;
        case BWD_W_TWIN:       rc = launch_gemm(pw, plan.w_tile, plan.w_layouts, stream); break;
        case BWD_COLSUM_FINAL: hipLaunchKernelGGL(k_colsum_final, dim3((c_out + 15) / 16), dim3(256), 0, stream, colsum, COLSUM_SPLITS, c_out, grad_b_l); break;
        case BWD_ZERO_ROWS:                                     // rows >= n_dst of grad_x start at zero
            hipLaunchKernelGGL(k_zero_rows, dim3(capped_grid((size_t)(n_src - (dims ? 0 : n_dst)) * c_in / 4 + 1, 256)), dim3(256), 0, stream, grad_x, c_in,
                               (int)n_dst, (int)n_src, n_dst_dev, n_src_dev);
            break;
        case BWD_X_TWIN:       rc = launch_gemm(px, plan.x_tile, plan.x_layouts, stream); break;
        case BWD_SCATTER_MEAN: hipLaunchKernelGGL(k_scatter_mean, scatter_grid, dim3(256), 0, stream, rowptr, col, (int)n_dst, gagg, c_in, grad_x, n_dst_dev); break;
        case BWD_DET_SUM:      enqueue_scatter_sum_det(rowptr, col, n_src, n_dst, nnz, gagg, c_in, grad_x, plan.det_vec, scratch, lay, dims, stream); break;
        case BWD_ORDERED:      enqueue_ordered_sum(rowptr, col, n_src, n_dst, nnz, arg, gagg, c_in, aggr, grad_x, plan.det_vec, scratch, lay, dims, stream); break;
        }
    }
    if (rc) return rc;
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

// The kernels sage_conv_backward launches for a layer of these capacities on a device of cu_count CUs, in launch order as a kernel
// trace shows them: backward_plan with at least one edge and the scratch sage_conv_scratch_bytes asks for.  Bit i < 8 of `misaligned`:
// field i of BwdAligned is not 16-byte aligned; bit 8: the call is sage_conv_backward_indexed (x is the feature matrix, read through n_id).
extern "C" int sage_backward_kernel_name_at(int64_t n_dst, int64_t n_src, int32_t c_in, int32_t c_out, int32_t need_grad_x, int32_t need_grad_b,
                                            int32_t cu_count, uint32_t misaligned, char *name, size_t cap) {
    clear_error();
    const bool indexed = misaligned >> 8 & 1u;
    POPE_REQUIRE(name && cap > 0 && n_dst > 0 && n_dst <= n_src && n_src < INT32_MAX && c_in > 0 && c_out > 0 && cu_count > 0 &&
                     misaligned < (1u << 9) && !(indexed && need_grad_x),
                 "sage_backward_kernel_name: bad argument");
    const auto ok = [misaligned](int bit) { return !(misaligned >> bit & 1u); };
    const BwdPlan p = backward_plan(n_dst, n_src, c_in, c_out, true, need_grad_x != 0, need_grad_b != 0, indexed,
                                    BwdAligned{ok(0), ok(1), ok(2), ok(3), ok(4), ok(5), ok(6), ok(7)}, cu_count,
                                    backward_scratch(n_src, n_dst, 0, c_in, c_out, g_sage_deterministic, indexed).slab_bytes);
    NameBuf names;
    for (int s = 0; s < p.n_steps; ++s) {
        switch (p.steps[s]) {
        case BWD_DUAL:               names.add("k_gemm_dual<64, 64, 2, 2>[splits=%d]", p.splits); break;
        case BWD_SCATTER_AND_FINALS: names.add("%s", "k_scatter_and_finals"); break;
        case BWD_FINALS:             names.add("%s", "k_bwd_finals"); break;
        case BWD_COLSUM_PARTIAL:     names.add("k_colsum_partial<%s>", p.colsum_vec ? "true" : "false"); break;
        case BWD_STREAMK:            names.add("k_gemm_streamk_tn<%d>%s+k_streamk_tn_fixup<%d>", SK_GK, p.xcd ? "[xcd]" : "", SK_GK); break;
        case BWD_GATHER_ROWS:        names.add("%s", "k_gather_rows"); break;        // (indexed calls only: bit 8 of the mask)
        case BWD_W_TWIN:             names.add_gemm(p.w_tile, p.w_layouts, p.splits); break;
        case BWD_COLSUM_FINAL:       names.add("%s", "k_colsum_final"); break;
        case BWD_ZERO_ROWS:          names.add("%s", "k_zero_rows"); break;
        case BWD_X_TWIN:             names.add_gemm(p.x_tile, p.x_layouts, 1); break;
        case BWD_SCATTER_MEAN:       names.add("%s", "k_scatter_mean"); break;
        case BWD_DET_SUM:
            names.add("k_det_clear+k_det_index<false>+k_det_scan+k_det_index<true>+k_scatter_sum_det<%s>", p.det_vec ? "true" : "false");
            break;
        case BWD_ORDERED: break;                                 // (sage_conv_backward_aggr's plan: this query plans the mean)
        }
    }
    return names.copy_to("sage_backward_kernel_name", name, cap);
}

extern "C" int sage_backward_kernel_name(int64_t n_dst, int64_t n_src, int32_t c_in, int32_t c_out, int32_t need_grad_x, int32_t need_grad_b,
                                         int32_t cu_count, char *name, size_t cap) {
    return sage_backward_kernel_name_at(n_dst, n_src, c_in, c_out, need_grad_x, need_grad_b, cu_count, 0, name, cap);
}

extern "C" int sage_conv_backward(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz,
                                  const float *x_src, const float *agg, int32_t c_in, const float *w_l, const float *w_r,
                                  int32_t c_out, const float *grad_out, float *grad_x, float *grad_w_l, float *grad_b_l,
                                  float *grad_w_r, void *scratch, size_t scratch_bytes, const int32_t *dims, void *stream_) {
    clear_error();
    POPE_REQUIRE(rowptr && (col || nnz == 0) && x_src && agg && w_l && w_r && grad_out && grad_w_l && grad_w_r && scratch,
                 "sage_conv_backward: null pointer");
    POPE_REQUIRE(n_dst > 0 && n_dst <= n_src && n_src < INT32_MAX && nnz >= 0 && c_in > 0 && c_out > 0, "sage_conv_backward: bad size");
    const BwdScratch lay = backward_scratch(n_src, n_dst, nnz, c_in, c_out, g_sage_deterministic, false);
    if (scratch_bytes < lay.total) {
        set_error("sage_conv_backward: scratch %zu < %zu bytes", scratch_bytes, lay.total);
        return POPE_ERR_WORKSPACE;
    }
    return conv_backward_impl(rowptr, col, n_src, n_dst, nnz, x_src, nullptr, agg, c_in, w_l, w_r, c_out, grad_out, grad_x, grad_w_l, grad_b_l,
                              grad_w_r, scratch, lay, dims, (hipStream_t)stream_);
}

// The backward pass of sage_conv_forward_indexed without a matrix of the destination rows: grad_w_r = grad_out^T x_dst reads
// x_dst[i] = feats[n_id[i]] through n_id in the weight-gradient kernel's loader (gemm_streamk_tn.h, rows1).  The input
// features have no gradient (layer 0), so there is no grad_x.  Scratch: sage_conv_backward_indexed_scratch_bytes.
extern "C" int sage_conv_backward_indexed(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst,
                                          int64_t nnz, const float *feats, int64_t n_rows, const float *agg, int32_t c_in, const float *w_l,
                                          const float *w_r, int32_t c_out, const float *grad_out, float *grad_w_l, float *grad_b_l,
                                          float *grad_w_r, void *scratch, size_t scratch_bytes, const int32_t *dims, void *stream_) {
    clear_error();
    POPE_REQUIRE(rowptr && (col || nnz == 0) && n_id && feats && agg && w_l && w_r && grad_out && grad_w_l && grad_w_r && scratch,
                 "sage_conv_backward_indexed: null pointer");
    POPE_REQUIRE(n_dst > 0 && n_dst <= n_src && n_src < INT32_MAX && n_rows > 0 && nnz >= 0 && c_in > 0 && c_out > 0,
                 "sage_conv_backward_indexed: bad size");
    const BwdScratch lay = backward_scratch(n_src, n_dst, nnz, c_in, c_out, g_sage_deterministic, true);
    if (scratch_bytes < lay.total) {
        set_error("sage_conv_backward_indexed: scratch %zu < %zu bytes", scratch_bytes, lay.total);
        return POPE_ERR_WORKSPACE;
    }
    return conv_backward_impl(rowptr, col, n_src, n_dst, nnz, feats, (const long long *)n_id, agg, c_in, w_l, w_r, c_out, grad_out, nullptr, grad_w_l,
                              grad_b_l, grad_w_r, scratch, lay, dims, (hipStream_t)stream_);
}

// ---- sum and max aggregation (include/graphpope_hip.h, "Sum and max aggregation"; the two kernels: aggregate.hip) ----
// The backward half on its own: the layer without columns, as sage_scatter_mean_det is for the mean -- the index at offset 0.
extern "C" size_t sage_aggregate_backward_scratch_size(int64_t n_src, int64_t n_dst, int64_t nnz) {
    return backward_scratch(n_src, n_dst, nnz, 0, 0, true, false).total;
}

// What the two backward entry points refuse about the aggregator before any HIP call.
static int aggr_backward_check(const char *who, int32_t aggr, const float *grad_x, const int32_t *arg) {
    POPE_REQUIRE(aggr == POPE_AGGR_ADD || aggr == POPE_AGGR_MAX, "%s: unknown aggr %d", who, aggr);
    POPE_REQUIRE(aggr != POPE_AGGR_MAX || !grad_x || arg, "%s: POPE_AGGR_MAX with a grad_x needs the arg the forward pass recorded", who);
    return POPE_OK;
}

extern "C" int sage_aggregate_backward(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, const int32_t *arg,
                                       const float *grad_agg, int32_t c, int32_t aggr, float *grad_x, void *scratch, size_t scratch_bytes,
                                       const int32_t *dims, void *stream_) {
    clear_error();
    int rc;
    if ((rc = aggr_backward_check("sage_aggregate_backward", aggr, grad_x, arg))) return rc;
    POPE_REQUIRE(n_src >= 0 && n_dst >= 0 && n_dst <= n_src && n_src < INT32_MAX && nnz >= 0 && nnz < INT32_MAX && c > 0,
                 "sage_aggregate_backward: bad size (destinations must be the first n_dst sources)");
    if (n_src == 0) return POPE_OK;
    POPE_REQUIRE(rowptr && (col || nnz == 0) && grad_agg && grad_x && scratch, "sage_aggregate_backward: null pointer");
    const BwdScratch lay = backward_scratch(n_src, n_dst, nnz, 0, 0, true, false);
    if (scratch_bytes < lay.total) {
        set_error("sage_aggregate_backward: scratch %zu < %zu bytes", scratch_bytes, lay.total);
        return POPE_ERR_WORKSPACE;
    }
    if (nnz == 0 && n_src == n_dst) return POPE_OK;                 // nothing to add and no row behind the destinations to overwrite
    enqueue_ordered_sum(rowptr, col, n_src, n_dst, nnz, arg, grad_agg, c, aggr, grad_x,
                        (c & 3) == 0 && aligned16(grad_agg) && aligned16(grad_x) && (aggr != POPE_AGGR_MAX || aligned16(arg)), scratch, lay, dims,
                        (hipStream_t)stream_);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

// conv_forward_run for sum and max: k_gather_reduce, then the projection conv_forward_run would launch behind its gather -- never the
// overlapped form, whose gather role is the mean's.  forward_plan is asked as for a call whose x_dst that form cannot write (the
// projections behind a gather do not look at that flag); the gather's own vector form is decided here.  The mean's runner is left
// exactly as it is: this one states the three projections behind a gather a second time.
static int conv_forward_run_aggr(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst, int64_t nnz,
                                 const float *x, int64_t x_rows, int32_t c_in, const float *w_l, const float *b_l, const float *w_r, int32_t c_out,
                                 float *agg, float *x_dst, float *out, void *scratch, size_t scratch_bytes, const int32_t *dims, BnStatsOut *stats,
                                 int aggr, int32_t *arg, hipStream_t stream) {
    int cus = 0, rc;
    if ((rc = device_cu_count(&cus))) return rc;
    const size_t rows_at = align_up(sage_conv_forward_scratch_bytes(n_dst, c_in, c_out), 256);   // the destination rows' place in the scratch buffer
    if (n_id && !x_dst) {                                            // no matrix of the destination rows from the caller: the projection wants one
        if (!scratch || scratch_bytes < rows_at + rows_matrix_bytes(n_dst, c_in)) {
            set_error("sage_conv_forward_indexed_aggr: without x_dst the scratch must hold sage_conv_forward_indexed_scratch_bytes (%zu), got %zu",
                      rows_at + rows_matrix_bytes(n_dst, c_in), scratch_bytes);
            return POPE_ERR_WORKSPACE;
        }
        x_dst = (float *)((char *)scratch + rows_at);
        scratch_bytes = rows_at;                                     // (what is left for the stream-K slabs)
    }
    const float *own = n_id ? x_dst : x;
    const bool gather_vec = (c_in & 3) == 0 && aligned16(x) && aligned16(agg) && aligned16(x_dst) && aligned16(arg);
    const FwdAligned al{aligned16(x), aligned16(agg), aligned16(own), false, aligned16(w_l), aligned16(w_r)};
    const FwdPlan plan = forward_plan(n_dst, c_in, c_out, x_rows, cus, al, scratch ? scratch_bytes : 0);
    enqueue_gather_reduce(rowptr, col, n_id, n_src, n_dst, nnz, x, x_rows, c_in, aggr, agg, arg, x_dst, gather_vec, dims, stream);
    switch (plan.path) {
    case FWD_TILE16:
        return gemm_tile16(agg, w_l, c_in, own, w_r, c_in, c_in, c_in, (int)n_dst, c_out, b_l, out, c_out, plan.rb, cus, stream, dims, stats);
    case FWD_STREAMK:
        return gemm_streamk(agg, w_l, c_in, own, w_r, c_in, c_in, c_in, (int)n_dst, c_out, b_l, out, c_out, scratch, cus, stream, dims);
    case FWD_OVERLAPPED:                                             // (not planned without x_dst_out)
    case FWD_PLAIN: break;
    }
    GemmArgs p = gemm_problem(Operand{agg, c_in, 1}, Operand{w_l, c_in, 1}, c_in, (int)n_dst, c_out, out, c_out);
    p.A1 = Operand{own, c_in, 1}; p.B1 = Operand{w_r, c_in, 1}; p.K1 = c_in;
    p.bias = b_l;
    p.m_dev = dims;
    return launch_gemm(p, plan.tile, plan.layouts, stream);
}

// The BatchNorm hand-off of the _aggr forward calls: all of it or none.
static int aggr_stats_check(const char *who, const double *bn_pa, const double *bn_pb, int32_t bn_parts_cap, const int32_t *bn_info) {
    const bool any = bn_pa || bn_pb || bn_info, all = bn_pa && bn_pb && bn_info && bn_parts_cap > 0;
    POPE_REQUIRE(!any || all, "%s: bn_pa, bn_pb and bn_info come together (with bn_parts_cap > 0) or are all NULL", who);
    return POPE_OK;
}

extern "C" int sage_conv_forward_aggr(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, const float *x_src,
                                      int32_t c_in, const float *w_l, const float *b_l, const float *w_r, int32_t c_out, float *agg, float *out,
                                      void *scratch, size_t scratch_bytes, const int32_t *dims, double *bn_pa, double *bn_pb, int32_t bn_parts_cap,
                                      int32_t *bn_info, int32_t aggr, int32_t *arg, void *stream_) {
    clear_error();
    int rc;
    POPE_REQUIRE(aggr_known(aggr), "sage_conv_forward_aggr: unknown aggr %d", aggr);
    if ((rc = aggr_stats_check("sage_conv_forward_aggr", bn_pa, bn_pb, bn_parts_cap, bn_info))) return rc;
    POPE_REQUIRE(rowptr && (col || nnz == 0) && x_src && w_l && w_r && agg && out, "sage_conv_forward_aggr: null pointer");
    POPE_REQUIRE(n_dst > 0 && n_dst <= n_src && n_src < INT32_MAX && nnz >= 0 && nnz < INT32_MAX && c_in > 0 && c_out > 0,
                 "sage_conv_forward_aggr: bad size (destinations must be the first n_dst sources)");
    BnStatsOut st{bn_pa, bn_pb, bn_parts_cap};
    if (aggr == POPE_AGGR_MEAN)                                     // forwarded: what sage_conv_forward / sage_conv_forward_stats run
        rc = conv_forward_run(rowptr, col, nullptr, n_dst, x_src, n_src, c_in, w_l, b_l, w_r, c_out, agg, nullptr, out, scratch, scratch_bytes, dims,
                              bn_pa ? &st : nullptr, (hipStream_t)stream_);
    else
        rc = conv_forward_run_aggr(rowptr, col, nullptr, n_src, n_dst, nnz, x_src, n_src, c_in, w_l, b_l, w_r, c_out, agg, nullptr, out, scratch,
                                   scratch_bytes, dims, bn_pa ? &st : nullptr, aggr, aggr == POPE_AGGR_MAX ? arg : nullptr, (hipStream_t)stream_);
    return bn_info ? stats_report(rc, st, bn_info) : rc;
}

extern "C" int sage_conv_forward_indexed_aggr(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst, int64_t nnz,
                                              const float *feats, int64_t n_rows, int32_t c_in, const float *w_l, const float *b_l, const float *w_r,
                                              int32_t c_out, float *agg, float *x_dst, float *out, void *scratch, size_t scratch_bytes,
                                              const int32_t *dims, double *bn_pa, double *bn_pb, int32_t bn_parts_cap, int32_t *bn_info, int32_t aggr,
                                              int32_t *arg, void *stream_) {
    clear_error();
    int rc;
    POPE_REQUIRE(aggr_known(aggr), "sage_conv_forward_indexed_aggr: unknown aggr %d", aggr);
    if ((rc = aggr_stats_check("sage_conv_forward_indexed_aggr", bn_pa, bn_pb, bn_parts_cap, bn_info))) return rc;
    POPE_REQUIRE(rowptr && (col || nnz == 0) && n_id && feats && w_l && w_r && agg && out, "sage_conv_forward_indexed_aggr: null pointer");
    POPE_REQUIRE(n_dst > 0 && n_dst <= n_src && n_src < INT32_MAX && n_rows > 0 && nnz >= 0 && nnz < INT32_MAX && c_in > 0 && c_out > 0,
                 "sage_conv_forward_indexed_aggr: bad size (destinations must be the first n_dst entries of n_id)");
    BnStatsOut st{bn_pa, bn_pb, bn_parts_cap};
    if (aggr == POPE_AGGR_MEAN)
        rc = conv_forward_run(rowptr, col, n_id, n_dst, feats, n_rows, c_in, w_l, b_l, w_r, c_out, agg, x_dst, out, scratch, scratch_bytes, dims,
                              bn_pa ? &st : nullptr, (hipStream_t)stream_);
    else
        rc = conv_forward_run_aggr(rowptr, col, n_id, n_src, n_dst, nnz, feats, n_rows, c_in, w_l, b_l, w_r, c_out, agg, x_dst, out, scratch,
                                   scratch_bytes, dims, bn_pa ? &st : nullptr, aggr, aggr == POPE_AGGR_MAX ? arg : nullptr, (hipStream_t)stream_);
    return bn_info ? stats_report(rc, st, bn_info) : rc;
}

// The index room is always in the size: the ordered sum is the only form of this pass's grad_x chain.
extern "C" size_t sage_conv_backward_aggr_scratch_size(int64_t n_src, int64_t n_dst, int64_t nnz, int32_t c_in, int32_t c_out) {
    const BwdScratch s = backward_scratch(n_src, n_dst, nnz, c_in, c_out, true, false);
    return s.core ? s.total : 0;
}

extern "C" int sage_conv_backward_aggr(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, const float *x_src,
                                       const float *agg, int32_t c_in, const float *w_l, const float *w_r, int32_t c_out, const float *grad_out,
                                       float *grad_x, float *grad_w_l, float *grad_b_l, float *grad_w_r, void *scratch, size_t scratch_bytes,
                                       const int32_t *dims, int32_t aggr, const int32_t *arg, void *stream_) {
    if (aggr == POPE_AGGR_MEAN)                                     // forwarded: the mean's pass, under the mode the library is in
        return sage_conv_backward(rowptr, col, n_src, n_dst, nnz, x_src, agg, c_in, w_l, w_r, c_out, grad_out, grad_x, grad_w_l, grad_b_l, grad_w_r,
                                  scratch, scratch_bytes, dims, stream_);
    clear_error();
    int rc;
    if ((rc = aggr_backward_check("sage_conv_backward_aggr", aggr, grad_x, arg))) return rc;
    POPE_REQUIRE(rowptr && (col || nnz == 0) && x_src && agg && w_l && w_r && grad_out && grad_w_l && grad_w_r && scratch,
                 "sage_conv_backward_aggr: null pointer");
    POPE_REQUIRE(n_dst > 0 && n_dst <= n_src && n_src < INT32_MAX && nnz >= 0 && nnz < INT32_MAX && c_in > 0 && c_out > 0,
                 "sage_conv_backward_aggr: bad size");
    const BwdScratch lay = backward_scratch(n_src, n_dst, nnz, c_in, c_out, true, false);
    if (scratch_bytes < lay.total) {
        set_error("sage_conv_backward_aggr: scratch %zu < %zu bytes", scratch_bytes, lay.total);
        return POPE_ERR_WORKSPACE;
    }
    return conv_backward_impl(rowptr, col, n_src, n_dst, nnz, x_src, nullptr, agg, c_in, w_l, w_r, c_out, grad_out, grad_x, grad_w_l, grad_b_l,
                              grad_w_r, scratch, lay, dims, (hipStream_t)stream_, aggr, aggr == POPE_AGGR_MAX ? arg : nullptr);
}

// ---- exact full-graph layer for inference: sage_full_layer_* (main.py:204-211 over all N nodes), included in place ----
#include "sage_full.h"

// ---- GCNConv on the whole graph: pope_gcn_* (project, then the normalised propagate, both passes), included in place ----
#include "gcn.h"

// ---- GATConv on the whole graph: pope_gat_* (project, edge softmax, attention propagate, both passes), included in place ----
#include "gat.h"

// ---- GATv2Conv on the whole graph: pope_gatv2_* (two projections, per-edge scores, edge softmax, gat.h's propagate, both passes) ----
#include "gatv2.h"
