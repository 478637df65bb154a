// GCNConv on the whole graph (included in place at the end of sage.hip, behind sage_full.h): project, then the normalised propagate.
//
//     out = A^ (x W) + b,   A^ = D^-1/2 (A + f I) D^-1/2   (PyG 1.7.0 GCNConv, its adj_t path; include/graphpope_hip.h: the contract)
// and, over the CSR by source with the SAME dinv (A^ is a symmetric scaling of A + f I, so A^T scales the same way):
//     t = A^T grad_out,   grad_weight = x^T t,   grad_x = t W^T,   grad_bias = column sums of grad_out.
//
//   k_gcn_degree_norm  one wave per row: dinv[i] = (float)(1 / sqrt((double)deg_i)), deg_i = the row's counted slots + f
//   k_gcn_transpose    W [c_in, c_out] as [c_out, c_in] in scratch: the whole-tile projection wants depth-contiguous operands
//   the projection     P [N, c_out] = x W by the GEMM machinery of sage.hip: whole tiles (gemm_tile16.h) under full_plan's conditions, else
//                      the plain tile kernel, which reads W where it lies (outer index contiguous)
//   k_gcn_clear        the two hub counters
//   k_gcn_propagate    k_full_aggregate's structure: one wave per (row, 256-column slab), ids 64 at a time with their dinv, both broadcast
//                      by shuffles, FULL_AHEAD rows in flight per lane (C <= 64: one column per lane and 32 rows in flight), term =
//                      dinv[j] * h[j] added in ascending slot order, then the finish (self term, dinv[i], bias).  A row longer than
//                      FULL_CHUNK slots goes onto the hub list.
//   k_gcn_hub_partial  one wave per (hub run of FULL_CHUNK slot positions, slab): the run's sum, into a partial row in scratch
//   k_gcn_hub_finish   one wave per (hub row, slab): the partials added in run order, then the same finish
// The backward pass adds the plain tile kernel twice (grad_weight with depth splits + k_slab_reduce, grad_x) and the two column-sum
// launches.  No float atomics anywhere; the hub launches are sized by capacity and read the counts on the device.
// Without dinv every weight is 1: x * 1.0f == x bit for bit, so there is one code path.
#pragma once

namespace pope {

struct GcnArgs {
    const int *rowptr, *col;
    int N, nnz, C;
    const float *dinv;                   // [N], or null: every weight is 1
    float self_w;                        // f: > 0 = slots with col == row are skipped and the row gets one self term of weight f
    const float *h;                      // [N, C]
    const float *bias;                   // [C], or null
    float *out;                          // [N, C]
    int *counters;                       // [0] hub rows, [1] hub chunks
    int *hubs;                           // [hub_cap][2]: row, first chunk (-1: its chunks did not fit -- an invalid CSR only)
    int *chunks;                         // [chunk_cap][2]: row, chunk of the row
    float *partial;                      // [chunk_cap, C]
    int hub_cap, chunk_cap;
};

// How a lane's columns lie.  VEC / scalar: full_load4's four columns per lane, FULL_AHEAD rows in flight.  NARROW (C <= 64, whatever
// the alignment): ONE column per lane and GCN_AHEAD_NARROW rows in flight -- a narrow row is one short load, and what a long row costs is
// its chain of round trips, not its bytes (measured at C = 7 on the Flickr-shaped graph: 237 us with 8 rows in flight, the 512-slot runs
// 64 round trips each).  The order of the additions is the same in all three.
constexpr int GCN_AHEAD_NARROW = 32;
template <bool NARROW> struct GcnForm { static constexpr int COLS = NARROW ? 1 : 4, AHEAD = NARROW ? GCN_AHEAD_NARROW : FULL_AHEAD; };

template <bool VEC, bool NARROW, int COLS>
__device__ __forceinline__ void gcn_load(const float *__restrict__ row, const int C, const int c0, const int lane, float (&r)[COLS]) {
    if constexpr (NARROW) r[0] = lane < C ? row[lane] : 0.f;
    else full_load4<VEC>(row, C, c0, lane, r);
}

template <bool VEC, bool NARROW, int COLS>
__device__ __forceinline__ void gcn_store(float *__restrict__ row, const int C, const int c0, const int lane, const float (&r)[COLS]) {
    if constexpr (NARROW) { if (lane < C) row[lane] = r[0]; }
    else full_store4<VEC>(row, C, c0, lane, r);
}

template <bool VEC, bool NARROW>
__device__ __forceinline__ int gcn_column(const int c0, const int lane, const int k) { return NARROW ? lane : full_column<VEC>(c0, lane, k); }

__device__ __forceinline__ void gcn_row_bounds(const GcnArgs &a, const int v, int &beg, int &end) {
    beg = min(max(a.rowptr[v], 0), a.nnz);
    end = min(max(a.rowptr[v + 1], beg), a.nnz);
}

// Every product and every sum below is rounded on its own (include/graphpope_hip.h: the summation contract), so no contraction.
#pragma clang fp contract(off)

// acc += dinv[col[p]] * h[col[p]] for the slots p = beg .. end - 1 of row v, strictly in that order.  An id outside [0, N) and, with
// skip_self, an id equal to v are not added (their lanes load row 0, which N > 0 makes valid, and drop it).
template <bool VEC, bool NARROW, int COLS>
__device__ __forceinline__ void gcn_add_slots(const GcnArgs &a, const int v, const int beg, const int end, const bool skip_self, const int c0,
                                              const int lane, float (&acc)[COLS]) {
    constexpr int AHEAD = GcnForm<NARROW>::AHEAD;
    const int C = a.C;
    for (int p0 = beg; p0 < end; p0 += 64) {
        int mine = p0 + lane < end ? a.col[p0 + lane] : -1;
        const bool ok = (unsigned)mine < (unsigned)a.N && !(skip_self && mine == v);
        if (!ok) mine = 0;
        const float w_mine = ok && a.dinv ? a.dinv[mine] : 1.0f;
        const unsigned long long live = __ballot(ok);
        const int cnt = min(64, end - p0);
        for (int t0 = 0; t0 < cnt; t0 += AHEAD) {
            float r[AHEAD][COLS], w[AHEAD];
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) {                        // past the end: the last slot again, loaded and not added
                const int t = min(t0 + u, cnt - 1);
                w[u] = __shfl(w_mine, t);
                gcn_load<VEC, NARROW>(a.h + (size_t)__shfl(mine, t) * C, C, c0, lane, r[u]);
            }
#pragma unroll
            for (int u = 0; u < AHEAD; ++u)
                if (t0 + u < cnt && (live >> (t0 + u) & 1ull)) {
#pragma unroll
                    for (int k = 0; k < COLS; ++k) {
                        const float term = w[u] * r[u][k];
                        acc[k] = acc[k] + term;
                    }
                }
        }
    }
}

// The finish of row v: + (dinv[v] * f) * h[v] with a self weight, * dinv[v] with dinv, + bias.
template <bool VEC, bool NARROW, int COLS>
__device__ __forceinline__ void gcn_finish(const GcnArgs &a, const int v, const int c0, const int lane, float (&acc)[COLS]) {
    const float dv = a.dinv ? a.dinv[v] : 1.0f;
    if (a.self_w > 0.f) {
        float own[COLS];
        gcn_load<VEC, NARROW>(a.h + (size_t)v * a.C, a.C, c0, lane, own);
        const float sw = dv * a.self_w;
#pragma unroll
        for (int k = 0; k < COLS; ++k) {
            const float term = sw * own[k];
            acc[k] = acc[k] + term;
        }
    }
#pragma unroll
    for (int k = 0; k < COLS; ++k) acc[k] = dv * acc[k];
    if (a.bias) {
#pragma unroll
        for (int k = 0; k < COLS; ++k) {
            const float b = a.bias[min(gcn_column<VEC, NARROW>(c0, lane, k), a.C - 1)];
            acc[k] = acc[k] + b;
        }
    }
}
#pragma clang fp contract(fast)

// dinv[i] = deg > 0 ? (float)(1 / sqrt((double)deg)) : 0 with deg = the counted slots of row i + self_w: with a self weight the slots
// whose id is i are not counted (the diagonal is replaced), every other slot is, ids out of range included.  One wave per row.
__global__ __launch_bounds__(256) void k_gcn_degree_norm(const int *__restrict__ rowptr, const int *__restrict__ col, const int N, const int nnz,
                                                         const float self_w, float *__restrict__ dinv) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int v = wave; v < N; v += nwaves) {
        const int beg = min(max(rowptr[v], 0), nnz), end = min(max(rowptr[v + 1], beg), nnz);
        int counted = end - beg;
        if (self_w > 0.f) {
            int own = 0;
            for (int p = beg + lane; p < end; p += 64) own += col[p] == v;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) own += __shfl_xor(own, d);
            counted -= own;
        }
        const double deg = (double)counted + (double)self_w;
        if (lane == 0) dinv[v] = deg > 0.0 ? (float)(1.0 / sqrt(deg)) : 0.f;
    }
}

// Wt [c_out, c_in] = W [c_in, c_out]^T (reads coalesced along c_out through a padded LDS tile, writes coalesced along c_in).
__global__ __launch_bounds__(256) void k_gcn_transpose(const float *__restrict__ W, const int c_in, const int c_out, float *__restrict__ Wt) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int tiles_o = (c_out + 31) / 32, tiles_i = (c_in + 31) / 32;
    for (int t = blockIdx.x; t < tiles_o * tiles_i; t += gridDim.x) {
        const int i0 = (t / tiles_o) * 32, o0 = (t % tiles_o) * 32;
#pragma unroll
        for (int r = ty; r < 32; r += 8)
            if (i0 + r < c_in && o0 + tx < c_out) tile[r][tx] = W[(size_t)(i0 + r) * c_out + o0 + tx];
        __syncthreads();
#pragma unroll
        for (int r = ty; r < 32; r += 8)
            if (o0 + r < c_out && i0 + tx < c_in) Wt[(size_t)(o0 + r) * c_in + i0 + tx] = tile[tx][r];
        __syncthreads();
    }
}

__global__ void k_gcn_clear(int *__restrict__ counters) {
    if (threadIdx.x < 2) counters[threadIdx.x] = 0;
}

template <bool VEC, bool NARROW>
__global__ __launch_bounds__(256) void k_gcn_propagate(const GcnArgs a) {
    constexpr int COLS = GcnForm<NARROW>::COLS;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int C = a.C, slabs = (C + 255) / 256;
    const int rows_stride = nwaves / slabs;
    const int slab = wave % slabs, first = wave / slabs;
    if (first >= rows_stride) return;
    const int c0 = slab * 256;
    const bool skip_self = a.self_w > 0.f;
    for (int v = first; v < a.N; v += rows_stride) {
        int beg, end;
        gcn_row_bounds(a, v, beg, end);
        const int deg = end - beg;
        if (deg > FULL_CHUNK) {                                      // a hub: onto the list (the wave of slab 0 alone), summed by the launches behind
            if (slab != 0) continue;
            const int nch = (deg + FULL_CHUNK - 1) / FULL_CHUNK;
            int idx = 0, base = 0;
            if (lane == 0) {
                idx = atomicAdd(&a.counters[0], 1);
                base = atomicAdd(&a.counters[1], nch);
            }
            idx = __shfl(idx, 0); base = __shfl(base, 0);
            if (idx < 0 || idx >= a.hub_cap) continue;
            const bool fits = base >= 0 && base <= a.chunk_cap - nch;
            if (lane == 0) { a.hubs[2 * idx] = v; a.hubs[2 * idx + 1] = fits ? base : -1; }
            if (fits)
                for (int k = lane; k < nch; k += 64) { a.chunks[2 * (base + k)] = v; a.chunks[2 * (base + k) + 1] = k; }
            continue;
        }
        float acc[COLS] = {};
        gcn_add_slots<VEC, NARROW>(a, v, beg, end, skip_self, c0, lane, acc);
        gcn_finish<VEC, NARROW>(a, v, c0, lane, acc);
        gcn_store<VEC, NARROW>(a.out + (size_t)v * C, C, c0, lane, acc);
    }
}

template <bool VEC, bool NARROW>
__global__ __launch_bounds__(256) void k_gcn_hub_partial(const GcnArgs a) {
    constexpr int COLS = GcnForm<NARROW>::COLS;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int C = a.C, slabs = (C + 255) / 256;
    const int count = min(max(a.counters[1], 0), a.chunk_cap);
    const long long items = (long long)count * slabs;
    const bool skip_self = a.self_w > 0.f;
    for (long long w = wave; w < items; w += nwaves) {
        const int e = (int)(w / slabs), c0 = (int)(w - (long long)e * slabs) * 256;
        const int v = a.chunks[2 * e], k = a.chunks[2 * e + 1];
        if ((unsigned)v >= (unsigned)a.N || k < 0) continue;        // (an entry nobody wrote: an invalid CSR only)
        int beg, end;
        gcn_row_bounds(a, v, beg, end);
        if ((long long)k * FULL_CHUNK >= end - beg) continue;
        beg += k * FULL_CHUNK;
        end = min(end, beg + FULL_CHUNK);
        float acc[COLS] = {};
        gcn_add_slots<VEC, NARROW>(a, v, beg, end, skip_self, c0, lane, acc);
        gcn_store<VEC, NARROW>(a.partial + (size_t)e * C, C, c0, lane, acc);
    }
}

template <bool VEC, bool NARROW>
__global__ __launch_bounds__(256) void k_gcn_hub_finish(const GcnArgs a) {
    constexpr int COLS = GcnForm<NARROW>::COLS;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int C = a.C, slabs = (C + 255) / 256;
    const int count = min(max(a.counters[0], 0), a.hub_cap);
    const long long items = (long long)count * slabs;
    for (long long w = wave; w < items; w += nwaves) {
        const int h = (int)(w / slabs), c0 = (int)(w - (long long)h * slabs) * 256;
        const int v = a.hubs[2 * h], base = a.hubs[2 * h + 1];
        if ((unsigned)v >= (unsigned)a.N || base < 0) continue;
        int beg, end;
        gcn_row_bounds(a, v, beg, end);
        const int deg = end - beg, nch = (deg + FULL_CHUNK - 1) / FULL_CHUNK;
        if (deg <= 0 || base > a.chunk_cap - nch) continue;
        float acc[COLS] = {};
        for (int k0 = 0; k0 < nch; k0 += 4) {                        // four partial rows in flight, added in run order
            float part[4][COLS];
#pragma unroll
            for (int u = 0; u < 4; ++u) gcn_load<VEC, NARROW>(a.partial + (size_t)(base + min(k0 + u, nch - 1)) * C, C, c0, lane, part[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (k0 + u < nch) {
#pragma unroll
                    for (int k = 0; k < COLS; ++k) acc[k] += part[u][k];
                }
        }
        gcn_finish<VEC, NARROW>(a, v, c0, lane, acc);
        gcn_store<VEC, NARROW>(a.out + (size_t)v * C, C, c0, lane, acc);
    }
}

// ---- where everything lies in the scratch buffers: laid out HERE and nowhere else (offsets are multiples of 256, a function of the sizes) ----
// The hub capacities are sage_full.h's: at most nnz / (FULL_CHUNK + 1) hubs, at most nnz / FULL_CHUNK + nnz / (FULL_CHUNK + 1) runs.
//   propagate:  counters int [2] | hubs int [hub_cap][2] | chunks int [chunk_cap][2] | partial [chunk_cap, C]
//   forward:    Wt [c_out, c_in] | P [N, c_out] | the propagate's region at width c_out
//   backward:   T [N, c_out] | slab [splits, c_in, c_out] | colsum [COLSUM_SPLITS, c_out] | the propagate's region at width c_out
struct GcnHubScratch {
    size_t counters, hubs, chunks, partial;
    int hub_cap, chunk_cap;
};
struct GcnScratch {
    size_t Wt, P, T, slab, colsum, total;
    GcnHubScratch hub;
};

static bool gcn_graph_ok(int64_t N, int64_t nnz) { return N > 0 && N < INT32_MAX && nnz >= 0 && nnz < INT32_MAX; }
static bool gcn_shape_ok(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out) { return gcn_graph_ok(N, nnz) && c_in > 0 && c_out > 0; }

// The weight gradient [c_in, c_out] reduces over the N rows: split that depth so the 64 x 128 tiles give ~400 blocks, each with at
// least four LDS stages of depth (weight_grad_splits for one result instead of two).
static int gcn_weight_splits(int64_t N, int c_in, int c_out) {
    const long long t = tiles(c_in, c_out, 64, 128);
    const int s = (int)std::min<long long>((400 + t - 1) / t, (N + 4 * GK - 1) / (4 * GK));
    return s < 1 ? 1 : s;
}

template <class Take>
static GcnHubScratch gcn_hub_scratch(Take &take, int64_t nnz, int32_t C) {
    GcnHubScratch s{};
    s.hub_cap = (int)(nnz / (FULL_CHUNK + 1));
    s.chunk_cap = s.hub_cap ? (int)(nnz / FULL_CHUNK + nnz / (FULL_CHUNK + 1)) : 0;
    s.counters = take(2 * sizeof(int));
    if (s.hub_cap) {
        s.hubs = take((size_t)s.hub_cap * 2 * sizeof(int));
        s.chunks = take((size_t)s.chunk_cap * 2 * sizeof(int));
        s.partial = take((size_t)s.chunk_cap * C * sizeof(float));
    }
    return s;
}

enum GcnCall { GCN_PROPAGATE, GCN_FORWARD, GCN_BACKWARD };

static GcnScratch gcn_scratch(GcnCall call, int64_t N, int64_t nnz, int32_t c_in, int32_t c_out) {
    GcnScratch s{};
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t was = at; at += align_up(bytes, 256); return was; };
    if (call == GCN_FORWARD) {
        s.Wt = take((size_t)c_out * c_in * sizeof(float));
        s.P = take((size_t)N * c_out * sizeof(float));
    } else if (call == GCN_BACKWARD) {
        s.T = take((size_t)N * c_out * sizeof(float));
        s.slab = take((size_t)gcn_weight_splits(N, c_in, c_out) * c_in * c_out * sizeof(float));
        s.colsum = take((size_t)COLSUM_SPLITS * c_out * sizeof(float));
    }
    s.hub = gcn_hub_scratch(take, nnz, c_out);
    s.total = at;
    return s;
}

// ---- which kernels a call runs: decided HERE; the lists below launch or print what this says (no HIP calls) ----
struct GcnAligned { bool x, weight, io, grad_x, scratch; };     // io: out (forward) / grad_out (backward)

struct GcnPlan {
    bool vec;              // the propagate kernels with 16-byte accesses
    bool narrow;           // ... or, for C <= 64, with one column per lane (vec is then false)
    bool hubs;             // a row can be longer than FULL_CHUNK: the clear and the two hub launches run
    // forward: the projection
    int rb;                // whole tiles: tile height / 16 (k_gcn_transpose in front); 0: the plain tile kernel
    GemmTile p_tile; GemmLayouts p_layouts;
    // backward
    int splits;            // depth splits of the weight gradient
    GemmTile w_tile; GemmLayouts w_layouts;
    bool need_grad_x;
    GemmTile x_tile; GemmLayouts x_layouts;
    bool colsum_vec;
};

// The propagate of [N, C] rows: h and out are the caller's (al_h, al_out) or lie in scratch.
static GcnPlan gcn_propagate_plan(int64_t nnz, int32_t C, bool al_h, bool al_out, bool al_scratch) {
    GcnPlan p{};
    p.narrow = C <= 64;
    p.vec = !p.narrow && (C & 3) == 0 && al_h && al_out && al_scratch;
    p.hubs = nnz > FULL_CHUNK;
    return p;
}

static GcnPlan gcn_forward_plan(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out, int cus, const GcnAligned &al) {
    GcnPlan p = gcn_propagate_plan(nnz, c_out, al.scratch, al.io, al.scratch);
    const int M = (int)N;
    const bool big = streamk_shape_ok(N, c_in, 0, c_out);
    if (big || (long long)M * c_out >= 64 * 1024) p.rb = t16_rb(M, M, c_out, c_in, 0, c_in, al.x && al.scratch, cus, !big);
    p.p_tile = gemm_tile_for(M, c_out, 1, 1);
    // x [N, c_in] depth-contiguous; W [c_in, c_out] read where it lies: outer index (the output column) contiguous
    p.p_layouts = gemm_layouts(pick_layout(al.x, c_in, 1, M, c_in), pick_layout(al.weight, 1, c_out, c_out, c_in), false, LAYOUT_GENERIC,
                               LAYOUT_GENERIC, false, LAYOUT_GENERIC);
    return p;
}

static GcnPlan gcn_backward_plan(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out, bool need_grad_x, const GcnAligned &al) {
    GcnPlan p = gcn_propagate_plan(nnz, c_out, al.io, al.scratch, al.scratch);
    const int M = (int)N;
    p.splits = gcn_weight_splits(N, c_in, c_out);
    p.w_tile = gemm_tile_for(c_in, c_out, p.splits, 1);
    // grad_weight[i, o] = sum_r x[r, i] t[r, o]: both operands outer-contiguous, depth = the rows
    p.w_layouts = gemm_layouts(pick_layout(al.x, 1, c_in, c_in, M), pick_layout(al.scratch, 1, c_out, c_out, M), false, LAYOUT_GENERIC,
                               LAYOUT_GENERIC, false, LAYOUT_GENERIC);
    p.need_grad_x = need_grad_x;
    p.x_tile = gemm_tile_for(M, c_in, 1, 1);
    // grad_x[r, i] = sum_o t[r, o] W[i, o]: both depth-contiguous
    p.x_layouts = gemm_layouts(pick_layout(al.scratch, c_out, 1, M, c_out), pick_layout(al.weight, c_out, 1, c_in, c_out), false, LAYOUT_GENERIC,
                               LAYOUT_GENERIC, false, LAYOUT_GENERIC);
    p.colsum_vec = (c_out & 3) == 0 && al.io;
    return p;
}

// ---- the launches of each call, written ONCE: the entry points run these lists, pope_gcn_kernel_name prints them (layer_host.h) ----
template <bool VEC, bool NARROW, class Sink>
static void gcn_propagate_as(Sink &s, const GcnArgs &a, bool hubs) {
    hub_family(s, hubs, k_gcn_clear, a, a.C, KName{"k_gcn_propagate<%s, %s>", tf(VEC), tf(NARROW)}, k_gcn_propagate<VEC, NARROW>,
               KName{"k_gcn_hub_partial<%s, %s>", tf(VEC), tf(NARROW)}, k_gcn_hub_partial<VEC, NARROW>,
               KName{"k_gcn_hub_finish<%s, %s>", tf(VEC), tf(NARROW)}, k_gcn_hub_finish<VEC, NARROW>);
}

template <class Sink>
static void gcn_propagate(Sink &s, const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *dinv, float self_w, const float *h,
                          int32_t C, const float *bias, float *out, const GcnHubScratch &lay, const GcnPlan &plan) {
    GcnArgs a{rowptr, col, (int)N, (int)nnz, C, dinv, self_w, h, bias, out};
    hub_bind(a, s, lay);
    if (plan.narrow) gcn_propagate_as<false, true>(s, a, plan.hubs);
    else if (plan.vec) gcn_propagate_as<true, false>(s, a, plan.hubs);
    else gcn_propagate_as<false, false>(s, a, plan.hubs);
}

template <class Sink>
static void gcn_forward(Sink &s, const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *dinv, float self_w, const float *x,
                        int32_t c_in, const float *weight, const float *bias, int32_t c_out, float *out, const GcnScratch &lay, const GcnPlan &plan) {
    float *Wt = s.floats(lay.Wt), *P = s.floats(lay.P);
    const dim3 tiles32(capped_grid((size_t)((c_in + 31) / 32) * ((c_out + 31) / 32) * 256, 256, 1024));
    // whole tiles want W depth-contiguous; the plain kernel reads it where it lies
    if (plan.rb) s.launch(KName{"k_gcn_transpose"}, k_gcn_transpose, tiles32, dim3(256), weight, c_in, c_out, Wt);
    project(s, x, c_in, (int)N, c_out, plan.rb ? Operand{Wt, c_in, 1} : Operand{weight, 1, c_out}, nullptr, P, plan.rb, plan.p_tile, plan.p_layouts);
    gcn_propagate(s, rowptr, col, N, nnz, dinv, self_w, P, c_out, bias, out, lay.hub, plan);
}

// want_bias: the bias gradient is asked for (the query: always).
template <class Sink>
static void gcn_backward(Sink &s, const int32_t *rowptr_t, const int32_t *col_t, int64_t N, int64_t nnz, const float *dinv, float self_w, const float *x,
                         int32_t c_in, const float *weight, int32_t c_out, const float *grad_out, float *grad_x, float *grad_weight, bool want_bias,
                         float *grad_bias, const GcnScratch &lay, const GcnPlan &plan) {
    float *T = s.floats(lay.T);
    gcn_propagate(s, rowptr_t, col_t, N, nnz, dinv, self_w, grad_out, c_out, nullptr, T, lay.hub, plan);
    split_depth_gemm(s, x, c_in, T, c_out, (int)N, grad_weight, plan.splits, s.floats(lay.slab), plan.w_tile, plan.w_layouts);
    if (plan.need_grad_x)
        s.gemm(gemm_problem(Operand{T, c_out, 1}, Operand{weight, c_out, 1}, c_out, (int)N, c_in, grad_x, c_in), plan.x_tile, plan.x_layouts);
    if (want_bias) s.colsum(grad_out, (int)N, c_out, s.floats(lay.colsum), plan.colsum_vec, grad_bias);
}

static bool gcn_self_weight_ok(float self_w) { return self_w >= 0.f && self_w <= 1e6f; }      // (false for a NaN)

}  // namespace pope

using namespace pope;

extern "C" int pope_gcn_degree_norm(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, float self_weight, float *dinv,
                                    void *stream) {
    clear_error();
    POPE_REQUIRE(rowptr && (col || nnz == 0) && dinv, "pope_gcn_degree_norm: null pointer");
    POPE_REQUIRE(gcn_graph_ok(N, nnz), "pope_gcn_degree_norm: bad size (N in (0, INT32_MAX), nnz in [0, INT32_MAX))");
    POPE_REQUIRE(gcn_self_weight_ok(self_weight), "pope_gcn_degree_norm: self_weight must be in [0, 1e6]");
    hipLaunchKernelGGL(k_gcn_degree_norm, dim3(capped_grid((size_t)N * 64, 256)), dim3(256), 0, (hipStream_t)stream, rowptr, col, (int)N, (int)nnz,
                       self_weight, dinv);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" size_t pope_gcn_propagate_scratch_size(int64_t N, int64_t nnz, int32_t C) {
    return gcn_shape_ok(N, nnz, 1, C) ? gcn_scratch(GCN_PROPAGATE, N, nnz, 1, C).total : 0;
}

extern "C" int pope_gcn_propagate(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *dinv, float self_weight,
                                  const float *h, int32_t C, const float *bias, float *out, void *scratch, size_t scratch_bytes, void *stream) {
    clear_error();
    POPE_REQUIRE(rowptr && (col || nnz == 0) && h && out && scratch, "pope_gcn_propagate: null pointer");
    POPE_REQUIRE(gcn_shape_ok(N, nnz, 1, C), "pope_gcn_propagate: bad size (N in (0, INT32_MAX), nnz in [0, INT32_MAX), C > 0)");
    POPE_REQUIRE(gcn_self_weight_ok(self_weight), "pope_gcn_propagate: self_weight must be in [0, 1e6]");
    POPE_REQUIRE(out != h, "pope_gcn_propagate: out must not alias h");
    const GcnScratch lay = gcn_scratch(GCN_PROPAGATE, N, nnz, 1, C);
    if (scratch_bytes < lay.total) return scratch_too_small("pope_gcn_propagate", scratch_bytes, lay.total);
    const GcnPlan plan = gcn_propagate_plan(nnz, C, aligned16(h), aligned16(out), aligned16(scratch));
    LaunchRun run{scratch, (hipStream_t)stream, 0};
    gcn_propagate(run, rowptr, col, N, nnz, dinv, self_weight, h, C, bias, out, lay.hub, plan);
    return run.done();
}

extern "C" size_t pope_gcn_conv_forward_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out) {
    return gcn_shape_ok(N, nnz, c_in, c_out) ? gcn_scratch(GCN_FORWARD, N, nnz, c_in, c_out).total : 0;
}

extern "C" int pope_gcn_conv_forward(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *dinv, float self_weight,
                                     const float *x, int32_t c_in, const float *weight, const float *bias, int32_t c_out, float *out,
                                     void *scratch, size_t scratch_bytes, void *stream_) {
    clear_error();
    POPE_REQUIRE(rowptr && (col || nnz == 0) && x && weight && out && scratch, "pope_gcn_conv_forward: null pointer");
    POPE_REQUIRE(gcn_shape_ok(N, nnz, c_in, c_out), "pope_gcn_conv_forward: bad size (N in (0, INT32_MAX), nnz in [0, INT32_MAX), c_in, c_out > 0)");
    POPE_REQUIRE(gcn_self_weight_ok(self_weight), "pope_gcn_conv_forward: self_weight must be in [0, 1e6]");
    const GcnScratch lay = gcn_scratch(GCN_FORWARD, N, nnz, c_in, c_out);
    if (scratch_bytes < lay.total) return scratch_too_small("pope_gcn_conv_forward", scratch_bytes, lay.total);
    int cus = 0, rc;
    if ((rc = device_cu_count(&cus))) return rc;
    const GcnPlan plan = gcn_forward_plan(N, nnz, c_in, c_out, cus, GcnAligned{aligned16(x), aligned16(weight), aligned16(out), true, aligned16(scratch)});
    LaunchRun run{scratch, (hipStream_t)stream_, cus};
    gcn_forward(run, rowptr, col, N, nnz, dinv, self_weight, x, c_in, weight, bias, c_out, out, lay, plan);
    return run.done();
}

extern "C" size_t pope_gcn_conv_backward_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out) {
    return gcn_shape_ok(N, nnz, c_in, c_out) ? gcn_scratch(GCN_BACKWARD, N, nnz, c_in, c_out).total : 0;
}

extern "C" int pope_gcn_conv_backward(const int32_t *rowptr_t, const int32_t *col_t, int64_t N, int64_t nnz, const float *dinv, float self_weight,
                                      const float *x, int32_t c_in, const float *weight, int32_t c_out, const float *grad_out, float *grad_x,
                                      float *grad_weight, float *grad_bias, void *scratch, size_t scratch_bytes, void *stream_) {
    clear_error();
    POPE_REQUIRE(rowptr_t && (col_t || nnz == 0) && x && weight && grad_out && grad_weight && scratch, "pope_gcn_conv_backward: null pointer");
    POPE_REQUIRE(gcn_shape_ok(N, nnz, c_in, c_out), "pope_gcn_conv_backward: bad size (N in (0, INT32_MAX), nnz in [0, INT32_MAX), c_in, c_out > 0)");
    POPE_REQUIRE(gcn_self_weight_ok(self_weight), "pope_gcn_conv_backward: self_weight must be in [0, 1e6]");
    const GcnScratch lay = gcn_scratch(GCN_BACKWARD, N, nnz, c_in, c_out);
    if (scratch_bytes < lay.total) return scratch_too_small("pope_gcn_conv_backward", scratch_bytes, lay.total);
    const GcnPlan plan = gcn_backward_plan(N, nnz, c_in, c_out, grad_x != nullptr,
                                           GcnAligned{aligned16(x), aligned16(weight), aligned16(grad_out), aligned16(grad_x), aligned16(scratch)});
    LaunchRun run{scratch, (hipStream_t)stream_, 0};
    gcn_backward(run, rowptr_t, col_t, N, nnz, dinv, self_weight, x, c_in, weight, c_out, grad_out, grad_x, grad_weight, grad_bias != nullptr, grad_bias, lay,
                 plan);
    return run.done();
}

// The launches of pope_gcn_conv_forward (backward = 0) or pope_gcn_conv_backward (backward != 0, with a bias gradient) for this shape on a
// device of cu_count CUs, in launch order: the lists above under the plan functions, printed.  Bit i of `misaligned`: operand i of {x, weight,
// out or grad_out, grad_x, scratch} is not 16-byte aligned.
extern "C" int pope_gcn_kernel_name(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out, int32_t backward, int32_t need_grad_x, int32_t cu_count,
                                    uint32_t misaligned, char *name, size_t cap) {
    clear_error();
    POPE_REQUIRE(name && cap > 0 && gcn_shape_ok(N, nnz, c_in, c_out) && cu_count > 0 && misaligned < (1u << 5), "pope_gcn_kernel_name: bad argument");
    const auto ok = [misaligned](int bit) { return !(misaligned >> bit & 1u); };
    const GcnAligned al{ok(0), ok(1), ok(2), ok(3), ok(4)};
    const GcnPlan p = backward ? gcn_backward_plan(N, nnz, c_in, c_out, need_grad_x != 0, al) : gcn_forward_plan(N, nnz, c_in, c_out, cu_count, al);
    LaunchNames names{cu_count};
    if (backward)
        gcn_backward(names, nullptr, nullptr, N, nnz, nullptr, 0.f, nullptr, c_in, nullptr, c_out, nullptr, nullptr, nullptr, true, nullptr,
                     gcn_scratch(GCN_BACKWARD, N, nnz, c_in, c_out), p);
    else
        gcn_forward(names, nullptr, nullptr, N, nnz, nullptr, 0.f, nullptr, c_in, nullptr, nullptr, c_out, nullptr,
                    gcn_scratch(GCN_FORWARD, N, nnz, c_in, c_out), p);
    return names.names.copy_to("pope_gcn_kernel_name", name, cap);
}
