// GATConv on the whole graph (included in place at the end of sage.hip, behind gcn.h): project, score, edge softmax, attention propagate.
//
//     h = x W^T viewed [N, H, C],  a_src = <h, att_l>,  a_dst = <h, att_r>,  e_p = leaky(a_src[j] + a_dst[i]) for the slot p = (j -> i),
//     alpha = softmax of e over the terms of row i,  agg[i, k, :] = sum_p alpha[p, k] h[j, k, :]      (PyG 1.7.0 GATConv on a single x;
//     include/graphpope_hip.h: the contract)
//
//   the projection        h [N, H C] = x W^T by the GEMM machinery of sage.hip (W [H C, c_in] is depth-contiguous where it lies: whole
//                         tiles need no transposed copy), into the CALLER's h: the backward pass reads it again
//   k_gat_scores          one thread per (row, head): a_src and a_dst, channels ascending
//   k_gat_attention       one wave per (row, head): the maximum, the sum of the exponentials, alpha of every slot and of the self term
//   k_gat_propagate       k_gcn_propagate's structure (one wave per (row, 256-column slab of H C), ids 64 at a time broadcast by shuffles,
//                         rows in flight) with the weight alpha[p, head(column)]; rows longer than FULL_CHUNK go onto gcn.h's hub list
//   k_gat_hub_partial / k_gat_hub_finish   the two capacity-sized launches behind it
//   k_gat_head_mean       concat = false: the head sum ascending, / (float)H, + bias
// Backward:
//   k_gat_spread_grad     concat = false: g[i, k, :] = grad_out[i, :] / (float)H
//   k_gat_edge_grad       one wave per (row, head), by destination: dalpha, t, then de [nnz, H], de_self and grad_a_dst
//   k_gat_src_grad        one wave per (source, head), by source through the slot map: grad_a_src
//   k_gat_propagate       over the CSR by source, alpha read through the slot map, rows = g, the finish adds grad_a_src att_l + grad_a_dst att_r
//   k_gat_att_partial + k_colsum_final twice   grad_att_l, grad_att_r (row slices, then the slices in order)
//   the plain tile kernel twice (grad_weight with depth splits + k_slab_reduce, grad_x), the two column-sum launches (grad_bias)
// No float atomics anywhere; the hub launches are sized by capacity and read the counts on the device.
#pragma once

namespace pope {

struct GatArgs {
    const int *rowptr, *col;
    int N, nnz, H, C, HC;
    const int *slot_map;                 // [nnz]: the slot of alpha that slot p of THIS CSR reads, or null: p itself
    const float *alpha;                  // [nnz, H]
    const float *alpha_self;             // [N, H], or null: no self term, and slots with col == row are ordinary
    const float *h;                      // [N, HC]: the rows that are summed
    const float *bias;                   // [HC], or null
    const float *ga_src, *ga_dst;        // [N, H] each, or null.  With them the finish adds ga_src[i, k] att_l[k, c] + ga_dst[i, k] att_r[k, c]
    const float *att_l, *att_r;          // [HC]
    float *out;                          // [N, HC]
    int *counters, *hubs, *chunks;       // gcn.h's hub list
    float *partial;                      // [chunk_cap, HC]
    int hub_cap, chunk_cap;
};

__device__ __forceinline__ void gat_row_bounds(const int *__restrict__ rowptr, const int nnz, const int v, int &beg, int &end) {
    beg = min(max(rowptr[v], 0), nnz);
    end = min(max(rowptr[v + 1], beg), nnz);
}

// The head of each of a lane's columns (a column past the end counts as the last: it is loaded as 0 and never stored).
template <bool VEC, bool NARROW, int COLS>
__device__ __forceinline__ void gat_heads(const GatArgs &a, const int c0, const int lane, int (&hd)[COLS]) {
#pragma unroll
    for (int k = 0; k < COLS; ++k) hd[k] = min(gcn_column<VEC, NARROW>(c0, lane, k), a.HC - 1) / a.C;
}

// Every product and every sum below is rounded on its own (include/graphpope_hip.h: the summation contract), so no contraction.
#pragma clang fp contract(off)

// acc += alpha[slot(p), head] * h[col[p]] for the slots p = beg .. end - 1 of row v, strictly in that order.  An id outside [0, N), a mapped
// slot outside [0, nnz) and, with a self term, an id equal to v are not added (their lanes load row 0 / slot 0 and drop them).
// one_head (the same for the whole wave): all of a lane's columns lie in one head, one weight load serves them.
template <bool VEC, bool NARROW, int COLS>
__device__ __forceinline__ void gat_add_slots(const GatArgs &a, const int v, const int beg, const int end, const int c0, const int lane,
                                              const int (&hd)[COLS], const bool one_head, float (&acc)[COLS]) {
    constexpr int AHEAD = GcnForm<NARROW>::AHEAD;
    const int HC = a.HC, H = a.H;
    const bool skip_self = a.alpha_self != nullptr;
    for (int p0 = beg; p0 < end; p0 += 64) {
        const int p = p0 + lane;
        int mine = p < end ? a.col[p] : -1;
        int slot = p < end ? (a.slot_map ? a.slot_map[p] : p) : -1;
        const bool ok = (unsigned)mine < (unsigned)a.N && (unsigned)slot < (unsigned)a.nnz && !(skip_self && mine == v);
        if (!ok) { mine = 0; slot = 0; }
        const unsigned long long live = __ballot(ok);
        const int cnt = min(64, end - p0);
        for (int t0 = 0; t0 < cnt; t0 += AHEAD) {
            float r[AHEAD][COLS], w[AHEAD][COLS];
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) {                        // past the end: the last slot again, loaded and not added
                const int t = min(t0 + u, cnt - 1);
                const float *__restrict__ wrow = a.alpha + (size_t)__shfl(slot, t) * H;
                if (one_head) {
                    const float w0 = wrow[hd[0]];
#pragma unroll
                    for (int k = 0; k < COLS; ++k) w[u][k] = w0;
                } else {
#pragma unroll
                    for (int k = 0; k < COLS; ++k) w[u][k] = wrow[hd[k]];
                }
                gcn_load<VEC, NARROW>(a.h + (size_t)__shfl(mine, t) * HC, HC, c0, lane, r[u]);
            }
#pragma unroll
            for (int u = 0; u < AHEAD; ++u)
                if (t0 + u < cnt && (live >> (t0 + u) & 1ull)) {
#pragma unroll
                    for (int k = 0; k < COLS; ++k) {
                        const float term = w[u][k] * r[u][k];
                        acc[k] = acc[k] + term;
                    }
                }
        }
    }
}

// The finish of row v: + alpha_self[v, head] * h[v] with a self term; + ga_src att_l, then + ga_dst att_r (the backward pass); + bias.
template <bool VEC, bool NARROW, int COLS>
__device__ __forceinline__ void gat_finish(const GatArgs &a, const int v, const int c0, const int lane, const int (&hd)[COLS], float (&acc)[COLS]) {
    if (a.alpha_self) {
        float own[COLS];
        gcn_load<VEC, NARROW>(a.h + (size_t)v * a.HC, a.HC, c0, lane, own);
#pragma unroll
        for (int k = 0; k < COLS; ++k) {
            const float term = a.alpha_self[(size_t)v * a.H + hd[k]] * own[k];
            acc[k] = acc[k] + term;
        }
    }
    if (a.ga_src) {
#pragma unroll
        for (int k = 0; k < COLS; ++k) {
            const int c = min(gcn_column<VEC, NARROW>(c0, lane, k), a.HC - 1);
            const float tl = a.ga_src[(size_t)v * a.H + hd[k]] * a.att_l[c];
            acc[k] = acc[k] + tl;
            const float tr = a.ga_dst[(size_t)v * a.H + hd[k]] * a.att_r[c];
            acc[k] = acc[k] + tr;
        }
    }
    if (a.bias) {
#pragma unroll
        for (int k = 0; k < COLS; ++k) {
            const float b = a.bias[min(gcn_column<VEC, NARROW>(c0, lane, k), a.HC - 1)];
            acc[k] = acc[k] + b;
        }
    }
}

// a_src[i, k] = sum_c h[i, k, c] * att_l[k, c], a_dst likewise with att_r: s = +0, then s = s + h * att for c ascending.  One thread per
// (row, head).
__global__ __launch_bounds__(256) void k_gat_scores(const float *__restrict__ h, const float *__restrict__ att_l, const float *__restrict__ att_r,
                                                    const int N, const int H, const int C, float *__restrict__ a_src, float *__restrict__ a_dst) {
    const long long items = (long long)N * H;
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < items; w += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(w % H);
        const float *__restrict__ row = h + w * C, *__restrict__ al = att_l + (size_t)k * C, *__restrict__ ar = att_r + (size_t)k * C;
        float sl = 0.f, sr = 0.f;
        for (int c = 0; c < C; ++c) {
            const float x = row[c];
            const float tl = x * al[c], tr = x * ar[c];
            sl = sl + tl;
            sr = sr + tr;
        }
        a_src[w] = sl;
        a_dst[w] = sr;
    }
}

__device__ __forceinline__ float gat_leaky(const float e, const float slope) { return e > 0.f ? e : slope * e; }

// The 64 lane values added by the xor butterfly 32, 16, .. 1: every lane ends with the same bits (each step adds the same two numbers).
__device__ __forceinline__ float gat_wave_sum(float s) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s = s + __shfl_xor(s, d);
    return s;
}

struct GatAttArgs {
    const int *rowptr, *col;
    int N, nnz, H;
    const float *a_src, *a_dst;          // [N, H]
    float slope;
    int self_loops;
    float *alpha, *alpha_self;           // [nnz, H], [N, H]
};

// One wave per (row i, head k).  The terms of the row: its slots with an id in [0, N) (with self loops: and not i), plus with self loops
// the self term.  m = their largest e' (exact); s: lane l adds exp(e' - m) of the slots beg + l, beg + l + 64, .. ascending from +0, the 64
// lane sums fold by the butterfly, then + the self term's exponential; alpha = exp(e' - m) / s.  Every other slot of the row gets 0.
__global__ __launch_bounds__(256) void k_gat_attention(const GatAttArgs a) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long items = (long long)a.N * a.H;
    const int H = a.H;
    for (long long w = wave; w < items; w += nwaves) {
        const int v = (int)(w / H), k = (int)(w - (long long)v * H);
        int beg, end;
        gat_row_bounds(a.rowptr, a.nnz, v, beg, end);
        const float ad = a.a_dst[w];
        const float es = a.self_loops ? gat_leaky(a.a_src[w] + ad, a.slope) : -INFINITY;
        float m = es;
        for (int p = beg + lane; p < end; p += 64) {
            const int j = a.col[p];
            if ((unsigned)j < (unsigned)a.N && !(a.self_loops && j == v)) m = fmaxf(m, gat_leaky(a.a_src[(size_t)j * H + k] + ad, a.slope));
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
        float s = 0.f;
        for (int p = beg + lane; p < end; p += 64) {
            const int j = a.col[p];
            if ((unsigned)j < (unsigned)a.N && !(a.self_loops && j == v)) s = s + expf(gat_leaky(a.a_src[(size_t)j * H + k] + ad, a.slope) - m);
        }
        s = gat_wave_sum(s);
        float xs = 0.f;
        if (a.self_loops) {
            xs = expf(es - m);
            s = s + xs;
        }
        for (int p = beg + lane; p < end; p += 64) {
            const int j = a.col[p];
            float al = 0.f;
            if ((unsigned)j < (unsigned)a.N && !(a.self_loops && j == v)) al = expf(gat_leaky(a.a_src[(size_t)j * H + k] + ad, a.slope) - m) / s;
            a.alpha[(size_t)p * H + k] = al;
        }
        if (lane == 0) a.alpha_self[w] = a.self_loops ? xs / s : 0.f;
    }
}

template <bool VEC, bool NARROW>
__global__ __launch_bounds__(256) void k_gat_propagate(const GatArgs a, const bool one_head) {
    constexpr int COLS = GcnForm<NARROW>::COLS;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int HC = a.HC, slabs = (HC + 255) / 256;
    const int rows_stride = nwaves / slabs;
    const int slab = wave % slabs, first = wave / slabs;
    if (first >= rows_stride) return;
    const int c0 = slab * 256;
    int hd[COLS];
    gat_heads<VEC, NARROW>(a, c0, lane, hd);
    for (int v = first; v < a.N; v += rows_stride) {
        int beg, end;
        gat_row_bounds(a.rowptr, a.nnz, v, beg, end);
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
        gat_add_slots<VEC, NARROW>(a, v, beg, end, c0, lane, hd, one_head, acc);
        gat_finish<VEC, NARROW>(a, v, c0, lane, hd, acc);
        gcn_store<VEC, NARROW>(a.out + (size_t)v * HC, HC, c0, lane, acc);
    }
}

template <bool VEC, bool NARROW>
__global__ __launch_bounds__(256) void k_gat_hub_partial(const GatArgs a, const bool one_head) {
    constexpr int COLS = GcnForm<NARROW>::COLS;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int HC = a.HC, slabs = (HC + 255) / 256;
    const int count = min(max(a.counters[1], 0), a.chunk_cap);
    const long long items = (long long)count * slabs;
    for (long long w = wave; w < items; w += nwaves) {
        const int e = (int)(w / slabs), c0 = (int)(w - (long long)e * slabs) * 256;
        const int v = a.chunks[2 * e], k = a.chunks[2 * e + 1];
        if ((unsigned)v >= (unsigned)a.N || k < 0) continue;        // (an entry nobody wrote: an invalid CSR only)
        int beg, end;
        gat_row_bounds(a.rowptr, a.nnz, v, beg, end);
        if ((long long)k * FULL_CHUNK >= end - beg) continue;
        beg += k * FULL_CHUNK;
        end = min(end, beg + FULL_CHUNK);
        int hd[COLS];
        gat_heads<VEC, NARROW>(a, c0, lane, hd);
        float acc[COLS] = {};
        gat_add_slots<VEC, NARROW>(a, v, beg, end, c0, lane, hd, one_head, acc);
        gcn_store<VEC, NARROW>(a.partial + (size_t)e * HC, HC, c0, lane, acc);
    }
}

template <bool VEC, bool NARROW>
__global__ __launch_bounds__(256) void k_gat_hub_finish(const GatArgs a) {
    constexpr int COLS = GcnForm<NARROW>::COLS;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int HC = a.HC, slabs = (HC + 255) / 256;
    const int count = min(max(a.counters[0], 0), a.hub_cap);
    const long long items = (long long)count * slabs;
    for (long long w = wave; w < items; w += nwaves) {
        const int hub = (int)(w / slabs), c0 = (int)(w - (long long)hub * slabs) * 256;
        const int v = a.hubs[2 * hub], base = a.hubs[2 * hub + 1];
        if ((unsigned)v >= (unsigned)a.N || base < 0) continue;
        int beg, end;
        gat_row_bounds(a.rowptr, a.nnz, v, beg, end);
        const int deg = end - beg, nch = (deg + FULL_CHUNK - 1) / FULL_CHUNK;
        if (deg <= 0 || base > a.chunk_cap - nch) continue;
        float acc[COLS] = {};
        for (int k0 = 0; k0 < nch; k0 += 4) {                        // four partial rows in flight, added in run order
            float part[4][COLS];
#pragma unroll
            for (int u = 0; u < 4; ++u) gcn_load<VEC, NARROW>(a.partial + (size_t)(base + min(k0 + u, nch - 1)) * HC, HC, c0, lane, part[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (k0 + u < nch) {
#pragma unroll
                    for (int k = 0; k < COLS; ++k) acc[k] = acc[k] + part[u][k];
                }
        }
        int hd[COLS];
        gat_heads<VEC, NARROW>(a, c0, lane, hd);
        gat_finish<VEC, NARROW>(a, v, c0, lane, hd, acc);
        gcn_store<VEC, NARROW>(a.out + (size_t)v * HC, HC, c0, lane, acc);
    }
}

// concat = false: out[i, c] = (agg[i, 0, c] + agg[i, 1, c] + ..  from +0, heads ascending) / (float)H (+ bias[c]).
__global__ __launch_bounds__(256) void k_gat_head_mean(const float *__restrict__ agg, const int N, const int H, const int C,
                                                       const float *__restrict__ bias, float *__restrict__ out) {
    const long long items = (long long)N * C;
    const float fh = (float)H;
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < items; w += (long long)gridDim.x * blockDim.x) {
        const long long i = w / C;
        const int c = (int)(w - i * C);
        float s = 0.f;
        for (int k = 0; k < H; ++k) s = s + agg[(i * H + k) * C + c];
        s = s / fh;
        if (bias) s = s + bias[c];
        out[w] = s;
    }
}

// concat = false, backward: g[i, k, c] = grad_out[i, c] / (float)H.
__global__ __launch_bounds__(256) void k_gat_spread_grad(const float *__restrict__ grad_out, const int N, const int H, const int C,
                                                         float *__restrict__ g) {
    const long long items = (long long)N * H * C;
    const float fh = (float)H;
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < items; w += (long long)gridDim.x * blockDim.x) {
        const long long i = w / ((long long)H * C);
        const int c = (int)(w % C);
        g[w] = grad_out[i * C + c] / fh;
    }
}

struct GatEdgeArgs {
    const int *rowptr, *col;
    int N, nnz, H, C;
    const float *a_src, *a_dst;          // [N, H]
    float slope;
    int self_loops;
    const float *alpha, *alpha_self;     // [nnz, H], [N, H]
    const float *h, *g;                  // [N, H C]
    float *de;                           // [nnz, H]
    float *de_self, *ga_dst;             // [N, H]
};

// <g[i, k, :], h[j, k, :]>: d = +0, then d = d + g * h for c ascending.
__device__ __forceinline__ float gat_dot(const float *__restrict__ gv, const float *__restrict__ hj, const int C) {
    float d = 0.f;
    for (int c = 0; c < C; ++c) {
        const float term = gv[c] * hj[c];
        d = d + term;
    }
    return d;
}

// One wave per (row i, head k), one lane per slot.  First dalpha_p of every term into de[p, k] and t = sum alpha_p dalpha_p (lane sums
// ascending, the butterfly, then the self term); then de_p = alpha_p (dalpha_p - t) * (e > 0 ? 1 : slope) over de[p, k] (0 for a slot that
// is no term), their sum (the same order) + de_self into ga_dst[i, k].
__global__ __launch_bounds__(256) void k_gat_edge_grad(const GatEdgeArgs a) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long items = (long long)a.N * a.H;
    const int H = a.H, C = a.C;
    const size_t HC = (size_t)H * C;
    for (long long w = wave; w < items; w += nwaves) {
        const int v = (int)(w / H), k = (int)(w - (long long)v * H);
        int beg, end;
        gat_row_bounds(a.rowptr, a.nnz, v, beg, end);
        const float *__restrict__ gv = a.g + (size_t)v * HC + (size_t)k * C;
        const float ad = a.a_dst[w];
        float t = 0.f;
        for (int p = beg + lane; p < end; p += 64) {
            const int j = a.col[p];
            float d = 0.f;
            if ((unsigned)j < (unsigned)a.N && !(a.self_loops && j == v)) {
                d = gat_dot(gv, a.h + (size_t)j * HC + (size_t)k * C, C);
                const float term = a.alpha[(size_t)p * H + k] * d;
                t = t + term;
            }
            a.de[(size_t)p * H + k] = d;
        }
        t = gat_wave_sum(t);
        float ds = 0.f, as = 0.f;
        if (a.self_loops) {
            ds = gat_dot(gv, a.h + (size_t)v * HC + (size_t)k * C, C);
            as = a.alpha_self[w];
            const float term = as * ds;
            t = t + term;
        }
        float sum = 0.f;
        for (int p = beg + lane; p < end; p += 64) {
            const int j = a.col[p];
            float x = 0.f;
            if ((unsigned)j < (unsigned)a.N && !(a.self_loops && j == v)) {
                const float e = a.a_src[(size_t)j * H + k] + ad;
                const float dd = a.de[(size_t)p * H + k] - t;
                x = a.alpha[(size_t)p * H + k] * dd;
                x = x * (e > 0.f ? 1.0f : a.slope);
                sum = sum + x;
            }
            a.de[(size_t)p * H + k] = x;
        }
        sum = gat_wave_sum(sum);
        float xs = 0.f;
        if (a.self_loops) {
            const float e = a.a_src[w] + ad;
            const float dd = ds - t;
            xs = as * dd;
            xs = xs * (e > 0.f ? 1.0f : a.slope);
            sum = sum + xs;
        }
        if (lane == 0) { a.de_self[w] = xs; a.ga_dst[w] = sum; }
    }
}

// grad_a_src[j, k] = the sum of de over the slots of row j of the CSR by source, read through the slot map (lane sums ascending, the
// butterfly), + de_self[j, k].  One wave per (source, head).
__global__ __launch_bounds__(256) void k_gat_src_grad(const int *__restrict__ rowptr_t, const int *__restrict__ slot_map, const int N, const int nnz,
                                                      const int H, const float *__restrict__ de, const float *__restrict__ de_self,
                                                      float *__restrict__ ga_src) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long items = (long long)N * H;
    for (long long w = wave; w < items; w += nwaves) {
        const int v = (int)(w / H), k = (int)(w - (long long)v * H);
        int beg, end;
        gat_row_bounds(rowptr_t, nnz, v, beg, end);
        float s = 0.f;
        for (int q = beg + lane; q < end; q += 64) {
            const int p = slot_map[q];
            if ((unsigned)p < (unsigned)nnz) s = s + de[(size_t)p * H + k];
        }
        s = gat_wave_sum(s);
        s = s + de_self[w];
        if (lane == 0) ga_src[w] = s;
    }
}

// part_l[slice, col] = sum over the slice's rows r ascending of ga_src[r, head(col)] * h[r, col], part_r with ga_dst: grid (column groups
// of 256, COLSUM_SPLITS row slices), one thread per column.  k_colsum_final adds the slices in order.
__global__ __launch_bounds__(256) void k_gat_att_partial(const float *__restrict__ h, const float *__restrict__ ga_src, const float *__restrict__ ga_dst,
                                                         const int N, const int H, const int C, float *__restrict__ part_l, float *__restrict__ part_r) {
    const int HC = H * C, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= HC) return;
    const int k = c / C;
    const int per = (N + (int)gridDim.y - 1) / (int)gridDim.y;
    const long long r0 = (long long)blockIdx.y * per, r1 = min((long long)N, r0 + per);
    float sl = 0.f, sr = 0.f;
    for (long long r = r0; r < r1; ++r) {
        const float x = h[r * HC + c];
        const float tl = ga_src[r * H + k] * x, tr = ga_dst[r * H + k] * x;
        sl = sl + tl;
        sr = sr + tr;
    }
    part_l[(size_t)blockIdx.y * HC + c] = sl;
    part_r[(size_t)blockIdx.y * HC + c] = sr;
}
#pragma clang fp contract(fast)

// slot_map[q] for slot q = (j -> i) of the CSR by source: the slot of the CSR by destination that holds the same edge -- the first j in row
// i (binary search: rows are ascending) plus q's rank among the equal ids of its own row.  -1 where the two CSRs do not match.  One wave
// per source row.
__global__ __launch_bounds__(256) void k_gat_slot_map(const int *__restrict__ rowptr, const int *__restrict__ col, const int *__restrict__ rowptr_t,
                                                      const int *__restrict__ col_t, const int N, const int nnz, int *__restrict__ slot_map) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int j = wave; j < N; j += nwaves) {
        int bt, et;
        gat_row_bounds(rowptr_t, nnz, j, bt, et);
        for (int q = bt + lane; q < et; q += 64) {
            const int i = col_t[q];
            int res = -1;
            if ((unsigned)i < (unsigned)N) {
                int lo = bt, hi = q;                                 // the first slot of row j that holds i: in [bt, q]
                while (lo < hi) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (col_t[mid] < i) lo = mid + 1; else hi = mid;
                }
                const int rank = q - lo;
                int b, e;
                gat_row_bounds(rowptr, nnz, i, b, e);
                int l2 = b, h2 = e;                                  // the first slot of row i (by destination) that holds j
                while (l2 < h2) {
                    const int mid = l2 + ((h2 - l2) >> 1);
                    if (col[mid] < j) l2 = mid + 1; else h2 = mid;
                }
                const long long r = (long long)l2 + rank;
                if (r < e && col[r] == j) res = (int)r;
            }
            slot_map[q] = res;
        }
    }
}

// ---- where everything lies in the scratch buffers: laid out HERE and nowhere else (offsets are multiples of 256, a function of the sizes) ----
//   propagate:  agg [N, HC] (concat = false only) | gcn.h's hub region at width HC
//   forward:    the propagate's
//   backward:   de [nnz, H] | de_self, ga_src, ga_dst [N, H] each | g [N, HC] (concat = false only) | GH [N, HC] | slab [splits, HC, c_in] |
//               part_l, part_r, colsum [COLSUM_SPLITS, HC] each | the hub region at width HC
struct GatScratch {
    size_t agg, de, de_self, ga_src, ga_dst, g, GH, slab, part_l, part_r, colsum, total;
    GcnHubScratch hub;
};

static bool gat_shape_ok(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C) {
    return gcn_graph_ok(N, nnz) && c_in > 0 && H > 0 && C > 0 && (int64_t)H * C <= INT32_MAX / 2;
}
static bool gat_slope_ok(float s) { return s >= 0.f && s <= 1.f; }                               // (false for a NaN)

enum GatCall { GAT_PROPAGATE, GAT_BACKWARD };

static GatScratch gat_scratch(GatCall call, int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, bool concat) {
    GatScratch s{};
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t was = at; at += align_up(bytes, 256); return was; };
    const size_t HC = (size_t)H * C;
    if (call == GAT_PROPAGATE) {
        if (!concat) s.agg = take((size_t)N * HC * sizeof(float));
    } else {
        s.de = take(std::max<size_t>((size_t)nnz, 1) * H * sizeof(float));
        s.de_self = take((size_t)N * H * sizeof(float));
        s.ga_src = take((size_t)N * H * sizeof(float));
        s.ga_dst = take((size_t)N * H * sizeof(float));
        if (!concat) s.g = take((size_t)N * HC * sizeof(float));
        s.GH = take((size_t)N * HC * sizeof(float));
        s.slab = take((size_t)gcn_weight_splits(N, (int)HC, c_in) * HC * c_in * sizeof(float));
        s.part_l = take((size_t)COLSUM_SPLITS * HC * sizeof(float));
        s.part_r = take((size_t)COLSUM_SPLITS * HC * sizeof(float));
        s.colsum = take((size_t)COLSUM_SPLITS * HC * sizeof(float));
    }
    s.hub = gcn_hub_scratch(take, nnz, (int32_t)HC);
    s.total = at;
    return s;
}

// ---- which kernels a call runs: decided HERE; the lists below launch or print what this says (no HIP calls) ----
struct GatAligned { bool x, weight, h, io, grad_x, scratch; };  // io: out (forward) / grad_out (backward)

struct GatPlan {
    bool vec, narrow, hubs, one_head;      // the propagate kernels (GcnPlan's three, and: a lane's columns lie in one head)
    bool concat;
    int rb;                                // forward: whole tiles (tile height / 16), or 0: the plain tile kernel
    GemmTile p_tile; GemmLayouts p_layouts;
    int splits;                            // backward
    GemmTile w_tile; GemmLayouts w_layouts;
    bool need_grad_x;
    GemmTile x_tile; GemmLayouts x_layouts;
    bool colsum_vec;
};

// The propagate of [N, H C] rows from `rows` to `out` (the hub partials lie in scratch).
static GatPlan gat_propagate_plan(int64_t nnz, int32_t H, int32_t C, bool concat, bool al_rows, bool al_out, bool al_scratch) {
    GatPlan p{};
    const int HC = H * C;
    p.narrow = HC <= 64;
    p.vec = !p.narrow && (HC & 3) == 0 && al_rows && al_out && al_scratch;
    p.hubs = nnz > FULL_CHUNK;
    p.one_head = p.narrow || (p.vec && (C & 3) == 0);
    p.concat = concat;
    return p;
}

static GatPlan gat_forward_plan(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, bool concat, int cus, const GatAligned &al) {
    GatPlan p = gat_propagate_plan(nnz, H, C, concat, al.h, concat ? al.io : al.scratch, al.scratch);
    const int M = (int)N, HC = H * C;
    const bool big = streamk_shape_ok(N, c_in, 0, HC);
    if (big || (long long)M * HC >= 64 * 1024) p.rb = t16_rb(M, M, HC, c_in, 0, c_in, al.x && al.weight, cus, !big);
    p.p_tile = gemm_tile_for(M, HC, 1, 1);
    // x [N, c_in] and W [HC, c_in]: both depth-contiguous
    p.p_layouts = gemm_layouts(pick_layout(al.x, c_in, 1, M, c_in), pick_layout(al.weight, c_in, 1, HC, c_in), false, LAYOUT_GENERIC, LAYOUT_GENERIC,
                               false, LAYOUT_GENERIC);
    return p;
}

static GatPlan gat_backward_plan(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, bool concat, bool need_grad_x, const GatAligned &al) {
    GatPlan p = gat_propagate_plan(nnz, H, C, concat, concat ? al.io : al.scratch, al.scratch, al.scratch);
    const int M = (int)N, HC = H * C;
    p.splits = gcn_weight_splits(N, HC, c_in);
    p.w_tile = gemm_tile_for(HC, c_in, p.splits, 1);
    // grad_weight[o, i] = sum_r GH[r, o] x[r, i]: both operands outer-contiguous, depth = the rows
    p.w_layouts = gemm_layouts(pick_layout(al.scratch, 1, HC, HC, M), pick_layout(al.x, 1, c_in, c_in, M), false, LAYOUT_GENERIC, LAYOUT_GENERIC, false,
                               LAYOUT_GENERIC);
    p.need_grad_x = need_grad_x;
    p.x_tile = gemm_tile_for(M, c_in, 1, 1);
    // grad_x[r, i] = sum_o GH[r, o] W[o, i]: GH depth-contiguous, W outer-contiguous
    p.x_layouts = gemm_layouts(pick_layout(al.scratch, HC, 1, M, HC), pick_layout(al.weight, 1, c_in, c_in, HC), false, LAYOUT_GENERIC, LAYOUT_GENERIC,
                               false, LAYOUT_GENERIC);
    const int wb = concat ? HC : C;
    p.colsum_vec = (wb & 3) == 0 && al.io;
    return p;
}

// ---- the launches of each call, written ONCE: the entry points run these lists, pope_gat_kernel_name prints them (layer_host.h) ----
template <bool VEC, bool NARROW, class Sink>
static void gat_propagate_as(Sink &s, const GatArgs &a, const GatPlan &plan) {
    hub_family(s, plan.hubs, k_gcn_clear, a, a.HC, KName{"k_gat_propagate<%s, %s>", tf(VEC), tf(NARROW)}, k_gat_propagate<VEC, NARROW>,
               KName{"k_gat_hub_partial<%s, %s>", tf(VEC), tf(NARROW)}, k_gat_hub_partial<VEC, NARROW>,
               KName{"k_gat_hub_finish<%s, %s>", tf(VEC), tf(NARROW)}, k_gat_hub_finish<VEC, NARROW>, plan.one_head);
}

template <class Sink>
static void gat_propagate(Sink &s, GatArgs a, const GcnHubScratch &lay, const GatPlan &plan) {
    hub_bind(a, s, lay);
    if (plan.narrow) gat_propagate_as<false, true>(s, a, plan);
    else if (plan.vec) gat_propagate_as<true, false>(s, a, plan);
    else gat_propagate_as<false, false>(s, a, plan);
}

// Steps 3 and 4 behind a given alpha: the propagate into out (concat) or into agg and from there the head mean.
template <class Sink>
static void gat_aggregate(Sink &s, const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *alpha, const float *alpha_self,
                          const float *h, int32_t H, int32_t C, const float *bias, float *out, const GatScratch &lay, const GatPlan &plan) {
    GatArgs a{};
    a.rowptr = rowptr; a.col = col; a.N = (int)N; a.nnz = (int)nnz; a.H = H; a.C = C; a.HC = H * C;
    a.alpha = alpha; a.alpha_self = alpha_self; a.h = h;
    a.bias = plan.concat ? bias : nullptr;
    a.out = plan.concat ? out : s.floats(lay.agg);
    gat_propagate(s, a, lay.hub, plan);
    if (!plan.concat) s.launch(KName{"k_gat_head_mean"}, k_gat_head_mean, dim3(capped_grid((size_t)N * C, 256)), dim3(256), a.out, (int)N, H, C, bias, out);
}

template <class Sink>
static void gat_attention(Sink &s, const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *h, int32_t H, int32_t C,
                          const float *att_l, const float *att_r, float slope, int self_loops, float *a_src, float *a_dst, float *alpha,
                          float *alpha_self) {
    s.launch(KName{"k_gat_scores"}, k_gat_scores, dim3(capped_grid((size_t)N * H, 256)), dim3(256), h, att_l, att_r, (int)N, H, C, a_src, a_dst);
    const GatAttArgs a{rowptr, col, (int)N, (int)nnz, H, a_src, a_dst, slope, self_loops, alpha, alpha_self};
    s.launch(KName{"k_gat_attention"}, k_gat_attention, dim3(capped_grid((size_t)N * H * 64, 256)), dim3(256), a);
}

template <class Sink>
static void gat_forward(Sink &s, const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *x, int32_t c_in, const float *weight,
                        const float *att_l, const float *att_r, const float *bias, int32_t H, int32_t C, float slope, int self_loops, float *h,
                        float *a_src, float *a_dst, float *alpha, float *alpha_self, float *out, const GatScratch &lay, const GatPlan &plan) {
    project(s, x, c_in, (int)N, H * C, Operand{weight, c_in, 1}, nullptr, h, plan.rb, plan.p_tile, plan.p_layouts);
    gat_attention(s, rowptr, col, N, nnz, h, H, C, att_l, att_r, slope, self_loops, a_src, a_dst, alpha, alpha_self);
    gat_aggregate(s, rowptr, col, N, nnz, alpha, self_loops ? alpha_self : nullptr, h, H, C, bias, out, lay, plan);
}

// concat = false: g[i, k, :] = grad_out[i, :] / (float)H in scratch at `at`; else grad_out itself.
template <class Sink>
static const float *gat_spread_grad(Sink &s, bool concat, const float *grad_out, int64_t N, int32_t H, int32_t C, size_t at) {
    if (concat) return grad_out;
    float *spread = s.floats(at);
    s.launch(KName{"k_gat_spread_grad"}, k_gat_spread_grad, dim3(capped_grid((size_t)N * H * C, 256)), dim3(256), grad_out, (int)N, H, C, spread);
    return spread;
}

// want_bias: the bias gradient is asked for (the query: always).
template <class Sink>
static void gat_backward(Sink &s, const int32_t *rowptr, const int32_t *col, const int32_t *rowptr_t, const int32_t *col_t, const int32_t *slot_map,
                         int64_t N, int64_t nnz, const float *x, int32_t c_in, const float *weight, const float *att_l, const float *att_r, int32_t H,
                         int32_t C, float slope, int self_loops, const float *h, const float *a_src, const float *a_dst, const float *alpha,
                         const float *alpha_self, const float *grad_out, float *grad_x, float *grad_weight, float *grad_att_l, float *grad_att_r,
                         bool want_bias, float *grad_bias, const GatScratch &lay, const GatPlan &plan) {
    const int HC = H * C;
    float *de = s.floats(lay.de), *de_self = s.floats(lay.de_self), *ga_src = s.floats(lay.ga_src), *ga_dst = s.floats(lay.ga_dst);
    float *GH = s.floats(lay.GH), *part_l = s.floats(lay.part_l), *part_r = s.floats(lay.part_r);
    const float *g = gat_spread_grad(s, plan.concat, grad_out, N, H, C, lay.g);
    const GatEdgeArgs ea{rowptr, col, (int)N, (int)nnz, H, C, a_src, a_dst, slope, self_loops, alpha, alpha_self, h, g, de, de_self, ga_dst};
    s.launch(KName{"k_gat_edge_grad"}, k_gat_edge_grad, dim3(capped_grid((size_t)N * H * 64, 256)), dim3(256), ea);
    s.launch(KName{"k_gat_src_grad"}, k_gat_src_grad, dim3(capped_grid((size_t)N * H * 64, 256)), dim3(256), rowptr_t, slot_map, (int)N, (int)nnz, H, de,
             de_self, ga_src);
    GatArgs a{};
    a.rowptr = rowptr_t; a.col = col_t; a.N = (int)N; a.nnz = (int)nnz; a.H = H; a.C = C; a.HC = HC;
    a.slot_map = slot_map; a.alpha = alpha; a.alpha_self = self_loops ? alpha_self : nullptr; a.h = g;
    a.ga_src = ga_src; a.ga_dst = ga_dst; a.att_l = att_l; a.att_r = att_r; a.out = GH;
    gat_propagate(s, a, lay.hub, plan);
    s.launch(KName{"k_gat_att_partial"}, k_gat_att_partial, dim3((HC + 255) / 256, COLSUM_SPLITS), dim3(256), h, ga_src, ga_dst, (int)N, H, C, part_l,
             part_r);
    s.launch(KName{"k_colsum_final"}, k_colsum_final, dim3((HC + 15) / 16), dim3(256), part_l, COLSUM_SPLITS, HC, grad_att_l);
    s.launch(KName{"k_colsum_final"}, k_colsum_final, dim3((HC + 15) / 16), dim3(256), part_r, COLSUM_SPLITS, HC, grad_att_r);
    split_depth_gemm(s, GH, HC, x, c_in, (int)N, grad_weight, plan.splits, s.floats(lay.slab), plan.w_tile, plan.w_layouts);
    if (plan.need_grad_x) s.gemm(gemm_problem(Operand{GH, HC, 1}, Operand{weight, 1, c_in}, HC, (int)N, c_in, grad_x, c_in), plan.x_tile, plan.x_layouts);
    if (want_bias) s.colsum(grad_out, (int)N, plan.concat ? HC : C, s.floats(lay.colsum), plan.colsum_vec, grad_bias);
}

static const char *const GAT_SIZE_MSG =              // (who, then "c_in, " for the calls that take c_in)
    "%s: bad size (N in (0, INT32_MAX), nnz in [0, INT32_MAX), %sH, C > 0, H C <= INT32_MAX / 2)";

}  // namespace pope

using namespace pope;

extern "C" int pope_gat_slot_map(const int32_t *rowptr, const int32_t *col, const int32_t *rowptr_t, const int32_t *col_t, int64_t N, int64_t nnz,
                                 int32_t *slot_map, void *stream) {
    clear_error();
    POPE_REQUIRE(rowptr && rowptr_t && ((col && col_t && slot_map) || nnz == 0), "pope_gat_slot_map: null pointer");
    POPE_REQUIRE(gcn_graph_ok(N, nnz), "pope_gat_slot_map: bad size (N in (0, INT32_MAX), nnz in [0, INT32_MAX))");
    if (nnz == 0) return POPE_OK;
    hipLaunchKernelGGL(k_gat_slot_map, dim3(capped_grid((size_t)N * 64, 256)), dim3(256), 0, (hipStream_t)stream, rowptr, col, rowptr_t, col_t, (int)N,
                       (int)nnz, slot_map);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" int pope_gat_attention(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *h, int32_t H, int32_t C,
                                  const float *att_l, const float *att_r, float negative_slope, int32_t add_self_loops, float *a_src, float *a_dst,
                                  float *alpha, float *alpha_self, void *stream) {
    clear_error();
    POPE_REQUIRE(rowptr && ((col && alpha) || nnz == 0) && h && att_l && att_r && a_src && a_dst && alpha_self, "pope_gat_attention: null pointer");
    POPE_REQUIRE(gat_shape_ok(N, nnz, 1, H, C), GAT_SIZE_MSG, "pope_gat_attention", "");
    POPE_REQUIRE(gat_slope_ok(negative_slope), "pope_gat_attention: negative_slope must be in [0, 1]");
    LaunchRun run{nullptr, (hipStream_t)stream, 0};
    gat_attention(run, rowptr, col, N, nnz, h, H, C, att_l, att_r, negative_slope, add_self_loops != 0, a_src, a_dst, alpha, alpha_self);
    return run.done();
}

extern "C" size_t pope_gat_propagate_scratch_size(int64_t N, int64_t nnz, int32_t H, int32_t C, int32_t concat) {
    return gat_shape_ok(N, nnz, 1, H, C) ? gat_scratch(GAT_PROPAGATE, N, nnz, 1, H, C, concat != 0).total : 0;
}

extern "C" int pope_gat_propagate(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *alpha, const float *alpha_self,
                                  const float *h, int32_t H, int32_t C, int32_t concat, const float *bias, float *out, void *scratch,
                                  size_t scratch_bytes, void *stream) {
    clear_error();
    POPE_REQUIRE(rowptr && ((col && alpha) || nnz == 0) && h && out && scratch, "pope_gat_propagate: null pointer");
    POPE_REQUIRE(gat_shape_ok(N, nnz, 1, H, C), GAT_SIZE_MSG, "pope_gat_propagate", "");
    POPE_REQUIRE(out != h, "pope_gat_propagate: out must not alias h");
    const GatScratch lay = gat_scratch(GAT_PROPAGATE, N, nnz, 1, H, C, concat != 0);
    if (scratch_bytes < lay.total) return scratch_too_small("pope_gat_propagate", scratch_bytes, lay.total);
    const GatPlan plan = gat_propagate_plan(nnz, H, C, concat != 0, aligned16(h), concat ? aligned16(out) : aligned16(scratch), aligned16(scratch));
    LaunchRun run{scratch, (hipStream_t)stream, 0};
    gat_aggregate(run, rowptr, col, N, nnz, alpha, alpha_self, h, H, C, bias, out, lay, plan);
    return run.done();
}

extern "C" size_t pope_gat_conv_forward_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, int32_t concat) {
    return gat_shape_ok(N, nnz, c_in, H, C) ? gat_scratch(GAT_PROPAGATE, N, nnz, c_in, H, C, concat != 0).total : 0;
}

extern "C" int pope_gat_conv_forward(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *x, int32_t c_in,
                                     const float *weight, const float *att_l, const float *att_r, const float *bias, int32_t H, int32_t C,
                                     int32_t concat, float negative_slope, int32_t add_self_loops, float *h, float *a_src, float *a_dst,
                                     float *alpha, float *alpha_self, float *out, void *scratch, size_t scratch_bytes, void *stream_) {
    clear_error();
    POPE_REQUIRE(rowptr && ((col && alpha) || nnz == 0) && x && weight && att_l && att_r && h && a_src && a_dst && alpha_self && out && scratch,
                 "pope_gat_conv_forward: null pointer");
    POPE_REQUIRE(gat_shape_ok(N, nnz, c_in, H, C), GAT_SIZE_MSG, "pope_gat_conv_forward", "c_in, ");
    POPE_REQUIRE(gat_slope_ok(negative_slope), "pope_gat_conv_forward: negative_slope must be in [0, 1]");
    const GatScratch lay = gat_scratch(GAT_PROPAGATE, N, nnz, c_in, H, C, concat != 0);
    if (scratch_bytes < lay.total) return scratch_too_small("pope_gat_conv_forward", scratch_bytes, lay.total);
    int cus = 0, rc;
    if ((rc = device_cu_count(&cus))) return rc;
    const GatPlan plan = gat_forward_plan(N, nnz, c_in, H, C, concat != 0, cus,
                                          GatAligned{aligned16(x), aligned16(weight), aligned16(h), aligned16(out), true, aligned16(scratch)});
    LaunchRun run{scratch, (hipStream_t)stream_, cus};
    gat_forward(run, rowptr, col, N, nnz, x, c_in, weight, att_l, att_r, bias, H, C, negative_slope, add_self_loops != 0, h, a_src, a_dst, alpha, alpha_self,
                out, lay, plan);
    return run.done();
}

extern "C" size_t pope_gat_conv_backward_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, int32_t concat) {
    return gat_shape_ok(N, nnz, c_in, H, C) ? gat_scratch(GAT_BACKWARD, N, nnz, c_in, H, C, concat != 0).total : 0;
}

extern "C" int pope_gat_conv_backward(const int32_t *rowptr, const int32_t *col, const int32_t *rowptr_t, const int32_t *col_t, const int32_t *slot_map,
                                      int64_t N, int64_t nnz, const float *x, int32_t c_in, const float *weight, const float *att_l,
                                      const float *att_r, int32_t H, int32_t C, int32_t concat, float negative_slope, int32_t add_self_loops,
                                      const float *h, const float *a_src, const float *a_dst, const float *alpha, const float *alpha_self,
                                      const float *grad_out, float *grad_x, float *grad_weight, float *grad_att_l, float *grad_att_r,
                                      float *grad_bias, void *scratch, size_t scratch_bytes, void *stream_) {
    clear_error();
    POPE_REQUIRE(rowptr && rowptr_t && ((col && col_t && slot_map && alpha) || nnz == 0) && x && weight && att_l && att_r && h && a_src && a_dst &&
                     alpha_self && grad_out && grad_weight && grad_att_l && grad_att_r && scratch,
                 "pope_gat_conv_backward: null pointer");
    POPE_REQUIRE(gat_shape_ok(N, nnz, c_in, H, C), GAT_SIZE_MSG, "pope_gat_conv_backward", "c_in, ");
    POPE_REQUIRE(gat_slope_ok(negative_slope), "pope_gat_conv_backward: negative_slope must be in [0, 1]");
    const bool cat = concat != 0;
    const GatScratch lay = gat_scratch(GAT_BACKWARD, N, nnz, c_in, H, C, cat);
    if (scratch_bytes < lay.total) return scratch_too_small("pope_gat_conv_backward", scratch_bytes, lay.total);
    const GatPlan plan = gat_backward_plan(N, nnz, c_in, H, C, cat, grad_x != nullptr,
                                           GatAligned{aligned16(x), aligned16(weight), aligned16(h), aligned16(grad_out), aligned16(grad_x),
                                                      aligned16(scratch)});
    LaunchRun run{scratch, (hipStream_t)stream_, 0};
    gat_backward(run, rowptr, col, rowptr_t, col_t, slot_map, N, nnz, x, c_in, weight, att_l, att_r, H, C, negative_slope, add_self_loops != 0, h, a_src,
                 a_dst, alpha, alpha_self, grad_out, grad_x, grad_weight, grad_att_l, grad_att_r, grad_bias != nullptr, grad_bias, lay, plan);
    return run.done();
}

// The launches of pope_gat_conv_forward (backward = 0) or pope_gat_conv_backward (backward != 0, with a bias gradient) for this shape on a
// device of cu_count CUs, in launch order: the lists above under the plan functions, printed.  Bit i of `misaligned`: operand i of {x, weight,
// h, out or grad_out, grad_x, scratch} is not 16-byte aligned.
extern "C" int pope_gat_kernel_name(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, int32_t concat, int32_t backward,
                                    int32_t need_grad_x, int32_t cu_count, uint32_t misaligned, char *name, size_t cap) {
    clear_error();
    POPE_REQUIRE(name && cap > 0 && gat_shape_ok(N, nnz, c_in, H, C) && cu_count > 0 && misaligned < (1u << 6), "pope_gat_kernel_name: bad argument");
    const auto ok = [misaligned](int bit) { return !(misaligned >> bit & 1u); };
    const GatAligned al{ok(0), ok(1), ok(2), ok(3), ok(4), ok(5)};
    const bool cat = concat != 0;
    const GatPlan p = backward ? gat_backward_plan(N, nnz, c_in, H, C, cat, need_grad_x != 0, al) : gat_forward_plan(N, nnz, c_in, H, C, cat, cu_count, al);
    LaunchNames names{cu_count};
    if (backward)
        gat_backward(names, nullptr, nullptr, nullptr, nullptr, nullptr, N, nnz, nullptr, c_in, nullptr, nullptr, nullptr, H, C, 0.f, 0, nullptr, nullptr,
                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true, nullptr,
                     gat_scratch(GAT_BACKWARD, N, nnz, c_in, H, C, cat), p);
    else
        gat_forward(names, nullptr, nullptr, N, nnz, nullptr, c_in, nullptr, nullptr, nullptr, nullptr, H, C, 0.f, 0, nullptr, nullptr, nullptr, nullptr,
                    nullptr, nullptr, gat_scratch(GAT_PROPAGATE, N, nnz, c_in, H, C, cat), p);
    return names.names.copy_to("pope_gat_kernel_name", name, cap);
}
