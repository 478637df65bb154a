// Exact full-graph SAGE layer for inference (included in place at the end of sage.hip): project, then aggregate, one epilogue.
//
// Replaces one pass of the layer loop at main.py:204-211 over ALL N nodes and ALL their neighbours:
//     out[v] = act( mean_{p in row v} x[col[p]] W_l^T + b_l + x[v] W_r^T ),   act = eval-mode BatchNorm + ReLU, or nothing
// The mean is linear, so the rows are projected FIRST (c_in -> c_out) and the projected rows are gathered: at 756 -> 256 the gather moves a
// third of the bytes.  Inference keeps nothing for a backward pass, which is what makes the order legal (include/graphpope_hip.h:
// sage_full_layer_forward, the contract and the summation order).
//
//   k_full_prepare     W = [W_l ; W_r] stacked and bias2 = [0 ; b_l] in scratch (x is then read ONCE by one product), rstd of the running
//                      variances, the two hub counters cleared
//   the projection     PR [N, 2 c_out] = x W^T + bias2 by the GEMM machinery of sage.hip: whole tiles (gemm_tile16.h) where the shape and
//                      the alignment qualify, else the plain tile kernel.  Row v of PR = P[v] | R[v].
//   k_full_aggregate   one wave per (destination row, 256-column slab): neighbour ids 64 at a time, broadcast by shuffles, FULL_AHEAD
//                      projected rows in flight per lane, the sum in ascending slot order, then * 1/deg, + R[v], BatchNorm, ReLU, one
//                      store.  A row longer than FULL_CHUNK slots is not summed here: its wave puts it on the hub list.
//   k_full_hub_partial one wave per (hub chunk of FULL_CHUNK slots, slab): the chunk's sum, into a partial row in scratch
//   k_full_hub_finish  one wave per (hub row, slab): the row's partials added in chunk order, then the same finish
// The hub launches are sized by capacity and read the true counts on the device; nothing is read back and no block waits for another.
// No float atomics anywhere: the order of the hub list does not reach the values.
#pragma once

namespace pope {

constexpr int FULL_CHUNK = 512;        // slots a wave sums on its own; include/graphpope_hip.h documents the value (the tests pin the order)
constexpr int FULL_AHEAD = 8;          // projected rows in flight per lane

// Column k of a lane's four: VEC lane l owns c0 + 4 l .. 4 l + 3 (one 16-byte access), otherwise c0 + l, l + 64, l + 128, l + 192.
template <bool VEC>
__device__ __forceinline__ int full_column(const int c0, const int lane, const int k) { return VEC ? c0 + 4 * lane + k : c0 + 64 * k + lane; }

template <bool VEC>
__device__ __forceinline__ void full_load4(const float *__restrict__ row, const int C, const int c0, const int lane, float (&r)[4]) {
    if (VEC) {
        const int c = c0 + 4 * lane;
        const float4 q = c < C ? *reinterpret_cast<const float4 *>(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        r[0] = q.x; r[1] = q.y; r[2] = q.z; r[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + 64 * k + lane;
            r[k] = c < C ? row[c] : 0.f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void full_store4(float *__restrict__ row, const int C, const int c0, const int lane, const float (&r)[4]) {
    if (VEC) {
        const int c = c0 + 4 * lane;
        if (c < C) *reinterpret_cast<float4 *>(row + c) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + 64 * k + lane;
            if (c < C) row[c] = r[k];
        }
    }
}

// acc += P[col[p]] for p = beg .. end - 1, strictly in that order.  P: rows of stride ld.  An id outside [0, N) reads row 0 (never followed).
template <bool VEC>
__device__ __forceinline__ void full_add_slots(const int *__restrict__ col, const int beg, const int end, const int N, const float *__restrict__ P,
                                               const long long ld, const int C, const int c0, const int lane, float (&acc)[4]) {
    for (int p0 = beg; p0 < end; p0 += 64) {
        int mine = p0 + lane < end ? col[p0 + lane] : 0;
        if ((unsigned)mine >= (unsigned)N) mine = 0;
        const int cnt = min(64, end - p0);
        for (int t0 = 0; t0 < cnt; t0 += FULL_AHEAD) {
            float r[FULL_AHEAD][4];
#pragma unroll
            for (int u = 0; u < FULL_AHEAD; ++u)                     // past the end: the last row again, loaded and not added
                full_load4<VEC>(P + (size_t)__shfl(mine, min(t0 + u, cnt - 1)) * ld, C, c0, lane, r[u]);
#pragma unroll
            for (int u = 0; u < FULL_AHEAD; ++u)
                if (t0 + u < cnt) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] += r[u][k];
                }
        }
    }
}

// The per-column BatchNorm parameters of a lane's four columns.
struct FullBn { float mean[4], rstd[4], gamma[4], beta[4]; };

template <bool VEC>
__device__ __forceinline__ void full_bn_load(FullBn &b, const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean,
                                             const float *__restrict__ rstd, const int C, const int c0, const int lane) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = min(full_column<VEC>(c0, lane, k), C - 1);
        b.mean[k] = mean[c]; b.rstd[k] = rstd[c]; b.gamma[k] = gamma[c]; b.beta[k] = beta[c];
    }
}

// The finish of a row: every operation rounded on its own, in the order the header documents (hipcc's default contraction would fuse
// s * inv + r into one fma: it is off for this function).  A NaN stays a NaN through the ReLU.
#pragma clang fp contract(off)
template <bool BN>
__device__ __forceinline__ void full_finish(float (&acc)[4], const float inv, const float (&r)[4], const FullBn &b) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float m = acc[k] * inv;
        float t = m + r[k];
        if (BN) {
            const float xhat = (t - b.mean[k]) * b.rstd[k];
            const float z = xhat * b.gamma[k];
            t = z + b.beta[k];
            t = t < 0.f ? 0.f : t;
        }
        acc[k] = t;
    }
}
#pragma clang fp contract(fast)

struct FullArgs {
    const int *rowptr, *col;
    int N, nnz, C;                       // C = c_out
    const float *PR;                     // [N, 2 C]: P | R
    const float *gamma, *beta, *mean, *rstd;
    float *out;
    int *counters;                       // [0] hub rows, [1] hub chunks
    int *hubs;                           // [hub_cap][2]: row, first chunk (-1: its chunks did not fit -- an invalid CSR only)
    int *chunks;                         // [chunk_cap][2]: row, chunk of the row
    float *partial;                      // [chunk_cap, C]
    int hub_cap, chunk_cap;
};

__device__ __forceinline__ void full_row_bounds(const FullArgs &a, const int v, int &beg, int &end) {
    beg = min(max(a.rowptr[v], 0), a.nnz);
    end = min(max(a.rowptr[v + 1], beg), a.nnz);
}

// W = [W_l ; W_r], bias2 = [0 ; b_l], rstd = (float)(1 / sqrt((double)var + eps)) (k_bn_final's eval-mode value), counters = 0.
__global__ __launch_bounds__(256) void k_full_prepare(const float *__restrict__ w_l, const float *__restrict__ w_r, const float *__restrict__ b_l,
                                                      const float *__restrict__ var, const float eps, const int c_in, const int c_out,
                                                      float *__restrict__ W, float *__restrict__ bias2, float *__restrict__ rstd, int *__restrict__ counters) {
    const size_t half = (size_t)c_out * c_in, stride = (size_t)gridDim.x * blockDim.x;
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = i0; i < 2 * half; i += stride) W[i] = i < half ? w_l[i] : w_r[i - half];
    for (size_t c = i0; c < 2 * (size_t)c_out; c += stride) bias2[c] = c >= (size_t)c_out && b_l ? b_l[c - c_out] : 0.f;
    if (var)
        for (size_t c = i0; c < (size_t)c_out; c += stride) rstd[c] = (float)(1.0 / sqrt((double)var[c] + (double)eps));
    if (i0 < 2) counters[i0] = 0;
}

// A wave owns one slab and every rows_stride-th row, so its BatchNorm parameters are loaded once.
template <bool VEC, bool BN>
__global__ __launch_bounds__(256) void k_full_aggregate(const FullArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int C = a.C, slabs = (C + 255) / 256;
    const int rows_stride = nwaves / slabs;
    const int slab = wave % slabs, first = wave / slabs;
    if (first >= rows_stride) return;
    const int c0 = slab * 256;
    const long long ld = 2ll * C;
    FullBn bn;
    if (BN) full_bn_load<VEC>(bn, a.gamma, a.beta, a.mean, a.rstd, C, c0, lane);
    for (int v = first; v < a.N; v += rows_stride) {
        int beg, end;
        full_row_bounds(a, v, beg, end);
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
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, r[4];
        full_add_slots<VEC>(a.col, beg, end, a.N, a.PR, ld, C, c0, lane, acc);
        full_load4<VEC>(a.PR + (size_t)v * ld + C, C, c0, lane, r);
        full_finish<BN>(acc, deg > 0 ? __fdiv_rn(1.0f, (float)deg) : 0.0f, r, bn);
        full_store4<VEC>(a.out + (size_t)v * C, C, c0, lane, acc);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_full_hub_partial(const FullArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int C = a.C, slabs = (C + 255) / 256;
    const int count = min(max(a.counters[1], 0), a.chunk_cap);
    const long long items = (long long)count * slabs;
    for (long long w = wave; w < items; w += nwaves) {
        const int e = (int)(w / slabs), c0 = (int)(w - (long long)e * slabs) * 256;
        const int v = a.chunks[2 * e], k = a.chunks[2 * e + 1];
        if ((unsigned)v >= (unsigned)a.N || k < 0) continue;        // (an entry nobody wrote: an invalid CSR only)
        int beg, end;
        full_row_bounds(a, v, beg, end);
        if ((long long)k * FULL_CHUNK >= end - beg) continue;
        beg += k * FULL_CHUNK;
        end = min(end, beg + FULL_CHUNK);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        full_add_slots<VEC>(a.col, beg, end, a.N, a.PR, 2ll * C, C, c0, lane, acc);
        full_store4<VEC>(a.partial + (size_t)e * C, C, c0, lane, acc);
    }
}

template <bool VEC, bool BN>
__global__ __launch_bounds__(256) void k_full_hub_finish(const FullArgs a) {
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
        full_row_bounds(a, v, beg, end);
        const int deg = end - beg, nch = (deg + FULL_CHUNK - 1) / FULL_CHUNK;
        if (deg <= 0 || base > a.chunk_cap - nch) continue;
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, r[4];
        for (int k0 = 0; k0 < nch; k0 += 4) {                        // four partial rows in flight, added in chunk order
            float part[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) full_load4<VEC>(a.partial + (size_t)(base + min(k0 + u, nch - 1)) * C, C, c0, lane, part[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (k0 + u < nch) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] += part[u][k];
                }
        }
        FullBn bn;
        if (BN) full_bn_load<VEC>(bn, a.gamma, a.beta, a.mean, a.rstd, C, c0, lane);
        full_load4<VEC>(a.PR + (size_t)v * 2 * C + C, C, c0, lane, r);
        full_finish<BN>(acc, __fdiv_rn(1.0f, (float)deg), r, bn);
        full_store4<VEC>(a.out + (size_t)v * C, C, c0, lane, acc);
    }
}

// ---- where everything lies in the scratch buffer: laid out HERE and nowhere else (offsets are multiples of 256, a function of the sizes) ----
//   W [2 c_out, c_in] | bias2 [2 c_out] | rstd [c_out] | counters int [2] | PR [N, 2 c_out] | hubs int [hub_cap][2] | chunks int [chunk_cap][2]
//   | partial [chunk_cap, c_out]
// A row is a hub with more than FULL_CHUNK slots, so there are at most nnz / (FULL_CHUNK + 1) of them, and a hub of d slots has
// ceil(d / FULL_CHUNK) <= d / FULL_CHUNK + d / (FULL_CHUNK + 1) chunks.
struct FullScratch {
    size_t W, bias2, rstd, counters, PR, hubs, chunks, partial, total;
    int hub_cap, chunk_cap;
};

static bool full_shape_ok(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out) {
    return N > 0 && N < INT32_MAX && nnz >= 0 && nnz < INT32_MAX && c_in > 0 && c_out > 0 && c_out <= INT32_MAX / 2;
}

static FullScratch full_scratch(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out) {
    FullScratch s{};
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t was = at; at += align_up(bytes, 256); return was; };
    s.hub_cap = (int)(nnz / (FULL_CHUNK + 1));
    s.chunk_cap = s.hub_cap ? (int)(nnz / FULL_CHUNK + nnz / (FULL_CHUNK + 1)) : 0;
    s.W = take(2 * (size_t)c_out * c_in * sizeof(float));
    s.bias2 = take(2 * (size_t)c_out * sizeof(float));
    s.rstd = take((size_t)c_out * sizeof(float));
    s.counters = take(2 * sizeof(int));
    s.PR = take((size_t)N * 2 * c_out * sizeof(float));
    if (s.hub_cap) {
        s.hubs = take((size_t)s.hub_cap * 2 * sizeof(int));
        s.chunks = take((size_t)s.chunk_cap * 2 * sizeof(int));
        s.partial = take((size_t)s.chunk_cap * c_out * sizeof(float));
    }
    s.total = at;
    return s;
}

// ---- which kernels the layer runs: decided HERE and nowhere else (no HIP calls) ----
// The projection takes the whole tiles of gemm_tile16.h under forward_plan's conditions (depth % 4, 16-byte-aligned x and scratch, 32-bit
// byte offsets, enough outputs), else the plain tile kernel in gemm_tile_for's tile.
struct FullPlan {
    int rb;                // whole tiles: tile height / 16; 0: the plain tile kernel
    GemmTile tile;
    GemmLayouts layouts;
    bool vec;              // the aggregate kernels with 16-byte accesses
    bool hubs;             // a row can be longer than FULL_CHUNK: the two hub launches run
};

static FullPlan full_plan(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out, int cus, bool al_x, bool al_out, bool al_scratch) {
    FullPlan p{};
    const int M = (int)N, NN = 2 * c_out;
    const bool big = streamk_shape_ok(N, c_in, 0, NN);
    if (big || (long long)M * NN >= 64 * 1024) p.rb = t16_rb(M, M, NN, c_in, 0, c_in, al_x && al_scratch, cus, !big);
    p.tile = gemm_tile_for(M, NN, 1, 1);
    p.layouts = gemm_layouts(pick_layout(al_x, c_in, 1, M, c_in), pick_layout(al_scratch, c_in, 1, NN, c_in), false, LAYOUT_GENERIC, LAYOUT_GENERIC,
                             false, LAYOUT_GENERIC);
    p.vec = (c_out & 3) == 0 && al_out && al_scratch;
    p.hubs = nnz > FULL_CHUNK;
    return p;
}

// ---- the launches of the layer, written ONCE: sage_full_layer_forward runs this list, sage_full_layer_kernel_name prints it (layer_host.h) ----
template <bool VEC, class Sink>
static void full_aggregate_as(Sink &s, const FullArgs &a, bool bn, bool hubs) {
    void (*const rows)(FullArgs) = bn ? k_full_aggregate<VEC, true> : k_full_aggregate<VEC, false>;
    void (*const partial)(FullArgs) = k_full_hub_partial<VEC>;
    void (*const finish)(FullArgs) = bn ? k_full_hub_finish<VEC, true> : k_full_hub_finish<VEC, false>;
    hub_family(s, hubs, nullptr /* k_full_prepare has cleared the counters */, a, a.C, KName{"k_full_aggregate<%s, %s>", tf(VEC), tf(bn)}, rows,
               KName{"k_full_hub_partial<%s>", tf(VEC)}, partial, KName{"k_full_hub_finish<%s, %s>", tf(VEC), tf(bn)}, finish);
}

// bn: the four BatchNorm pointers are given (the query: has_bn).
template <class Sink>
static void full_layer(Sink &s, const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *x, int32_t c_in, const float *w_l,
                      const float *b_l, const float *w_r, int32_t c_out, const float *bn_gamma, const float *bn_beta, const float *bn_mean,
                      const float *bn_var, float bn_eps, bool bn, float *out, const FullScratch &lay, const FullPlan &plan) {
    float *W = s.floats(lay.W), *bias2 = s.floats(lay.bias2), *rstd = s.floats(lay.rstd), *PR = s.floats(lay.PR);
    s.launch(KName{"k_full_prepare"}, k_full_prepare, dim3(capped_grid(2 * (size_t)c_out * c_in, 256, 1024)), dim3(256), w_l, w_r, b_l, bn_var, bn_eps,
             c_in, c_out, W, bias2, rstd, s.ints(lay.counters));
    project(s, x, c_in, (int)N, 2 * c_out, Operand{W, c_in, 1}, bias2, PR, plan.rb, plan.tile, plan.layouts);
    FullArgs a{rowptr, col, (int)N, (int)nnz, c_out, PR, bn_gamma, bn_beta, bn_mean, rstd, out};
    hub_bind(a, s, lay);
    if (plan.vec) full_aggregate_as<true>(s, a, bn, plan.hubs);
    else full_aggregate_as<false>(s, a, bn, plan.hubs);
}

}  // namespace pope

using namespace pope;

// main.py:204-211, one pass of the layer loop over the whole graph: the bytes the call needs (0: a shape it refuses).
extern "C" size_t sage_full_layer_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out) {
    return full_shape_ok(N, nnz, c_in, c_out) ? full_scratch(N, nnz, c_in, c_out).total : 0;
}

// main.py:204-211: x = convs[i]((x, x), adj_t) over every node and every neighbour, then bns[i](x).relu_() in eval mode if the four
// BatchNorm pointers are given (dropout is the identity there).
extern "C" int sage_full_layer_forward(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *x, int32_t c_in,
                                       const float *w_l, const float *b_l, const float *w_r, int32_t c_out, const float *bn_gamma,
                                       const float *bn_beta, const float *bn_mean, const float *bn_var, float bn_eps, float *out, void *scratch,
                                       size_t scratch_bytes, void *stream_) {
    clear_error();
    POPE_REQUIRE(rowptr && (col || nnz == 0) && x && w_l && w_r && out && scratch, "sage_full_layer_forward: null pointer");
    POPE_REQUIRE(full_shape_ok(N, nnz, c_in, c_out), "sage_full_layer_forward: bad size (N and nnz in [0, INT32_MAX), N > 0, 0 < c_out <= INT32_MAX / 2)");
    const int given = (bn_gamma != nullptr) + (bn_beta != nullptr) + (bn_mean != nullptr) + (bn_var != nullptr);
    POPE_REQUIRE(given == 0 || given == 4, "sage_full_layer_forward: the four BatchNorm pointers go together (%d of 4 given)", given);
    const FullScratch lay = full_scratch(N, nnz, c_in, c_out);
    if (scratch_bytes < lay.total) return scratch_too_small("sage_full_layer_forward", scratch_bytes, lay.total);
    int cus = 0, rc;
    if ((rc = device_cu_count(&cus))) return rc;
    const FullPlan plan = full_plan(N, nnz, c_in, c_out, cus, aligned16(x), aligned16(out), aligned16(scratch));
    LaunchRun run{scratch, (hipStream_t)stream_, cus};
    full_layer(run, rowptr, col, N, nnz, x, c_in, w_l, b_l, w_r, c_out, bn_gamma, bn_beta, bn_mean, bn_var, bn_eps, given == 4, out, lay, plan);
    return run.done();
}

// The launches of the call above (main.py:204-211 for a layer of this shape) on a device of cu_count CUs, as a kernel trace shows them:
// full_layer's list under full_plan, printed.  Bit i of `misaligned`: operand i of {x, out, scratch} is not 16-byte aligned (the weights are
// copied by scalar accesses: their alignment changes nothing).
extern "C" int sage_full_layer_kernel_name(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out, int32_t has_bn, int32_t cu_count,
                                           uint32_t misaligned, char *name, size_t cap) {
    clear_error();
    POPE_REQUIRE(name && cap > 0 && full_shape_ok(N, nnz, c_in, c_out) && cu_count > 0 && misaligned < (1u << 3),
                 "sage_full_layer_kernel_name: bad argument");
    const auto ok = [misaligned](int bit) { return !(misaligned >> bit & 1u); };
    const FullPlan p = full_plan(N, nnz, c_in, c_out, cu_count, ok(0), ok(1), ok(2));
    LaunchNames names{cu_count};
    full_layer(names, nullptr, nullptr, N, nnz, nullptr, c_in, nullptr, nullptr, nullptr, c_out, nullptr, nullptr, nullptr, nullptr, 0.f, has_bn != 0,
               nullptr, full_scratch(N, nnz, c_in, c_out), p);
    return names.names.copy_to("sage_full_layer_kernel_name", name, cap);
}
