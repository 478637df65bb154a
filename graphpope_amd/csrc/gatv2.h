// GATv2Conv on the whole graph (included in place at the end of sage.hip, behind gat.h): project twice, score every edge, edge softmax,
// attention propagate.
//
//     hl = x W_l^T + b_l,  hr = x W_r^T + b_r  viewed [N, H, C],   z_p = hl[j] + hr[i] for the slot p = (j -> i),
//     e_p[k] = sum_c att[k, c] leaky(z_p[k, c]),   alpha = softmax of e over the terms of row i,   agg[i, k, :] = sum_p alpha[p, k] hl[j, k, :]
//     (PyG GATv2Conv on a single x; include/graphpope_hip.h: the contract.)  The score is not a sum of two per-node scalars: every
//     (slot, head) is a C-wide dot product over a gathered row, and no [nnz, H, C] tensor is ever written.
//
//   the projections       the GEMM machinery of sage.hip with the linear bias in the epilogue, into the CALLER's hl and hr (one product
//                         with shared weights: hr is hl)
//   k_gatv2_scores        one wave per run of V2_GROUP slot positions (hub rows are cut like every other row: a slot's score depends on
//                         no other slot), then one wave per row for the self term.  Lanes over the H C columns: lane l of a 256-column
//                         slab owns the columns 4 l .. 4 l + 3 (one 16-byte load where pointers and H C allow, four 4-byte loads
//                         otherwise: the SAME columns), hr[i] and att in registers, one coalesced gather of hl[j] per slot, 8 rows
//                         in flight (4 or 2 in the rarer forms: v2_ahead), and a segmented fold over the lanes of each head.  DOT = true: the same walk with the product
//                         g[i] * hl[j] in the term's place (dalpha of the backward pass).
//   k_gatv2_softmax       one wave per (row, head) over a given e: k_gat_attention's order (lane sums ascending, the xor butterfly, then
//                         the self term), expf.  alpha may be e, alpha_self may be e_self.
//   the aggregate         gat.h's propagate (k_gat_propagate and its hub launches, k_gat_head_mean) over hl, unchanged
// Backward:
//   k_gat_spread_grad     concat = false
//   k_gatv2_scores<DOT>   dalpha [nnz, H], dalpha_self [N, H]
//   k_gatv2_edge_grad     one wave per (row, head): t = sum alpha dalpha, de = alpha (dalpha - t) in place, slots and self term
//   k_gatv2_rowsum<SRC = false>   by destination: grad_hr[i] and the row's part of grad_att (a second gather of hl[j]); k_gat_propagate's
//                         structure, rows longer than FULL_CHUNK on gcn.h's hub list (k_gatv2_hub_partial / k_gatv2_hub_finish)
//   k_gatv2_rowsum<SRC = true>    by source through the slot map: grad_hl[j] (two row gathers per slot: hr[i] and g[i]); the same launch family
//   k_colsum_partial + k_colsum_final   grad_att from the rows' parts, the linear-bias gradients, grad_bias
//   k_gatv2_add           shared weights: grad_hl += grad_hr
//   the plain tile kernel  grad_lin_l.weight, grad_lin_r.weight (depth splits + k_slab_reduce), grad_x (ONE launch: the sum of two products)
// No float atomics anywhere; the hub launches are sized by capacity and read the counts on the device.
//
// THE ORDER OF e (identical for every row, hub or not, and for the 16-byte and the 4-byte loads; DOT alike with its own term):
//   t[c] = att[c] * leaky(hl[j, c] + hr[i, c]),  leaky(z) = z > 0 ? z : slope * z  (each operation rounded on its own).
//   The columns are cut into slabs of 256; in a slab, lane l (0 .. 63) holds the columns c0 + 4 l + q, q = 0 .. 3.
//   C % 4 == 0 (a lane's columns lie in one head):  u[l] = ((t0 + t1) + t2) + t3, then for d = 1, 2, 4, 8, 16, 32:
//       u[l] = u[l] + u[l + d]  where l + d < 64 and column c0 + 4 (l + d) exists and lies in the head of lane l  (all lanes at once);
//       the head's part P of the slab is u of its first lane in the slab.
//   otherwise: four planes, plane q holding t[c0 + 4 l + q] in lane l, each folded on its own by the same rule; the head's part
//       P = ((P0 + P1) + P2) + P3, Pq = the folded value of the head's first lane in plane q, +0 for a plane without a column of the head.
//   e[k] = P of the head's first slab, then e = e + P for its further slabs ascending.
#pragma once

namespace pope {

// Gathered rows in flight per lane in the score pass: 8 in the common form (C % 4 == 0, H C <= 256), 4 in the four-plane and in the
// many-slab form and 2 where both meet: their per-slot state (four planes, a carry per slot) does not fit the scalar registers at 8.
constexpr int v2_ahead(bool one_head, bool single) { return one_head && single ? 8 : one_head || single ? 4 : 2; }
constexpr int V2_ROW_AHEAD = 4;        // ... of the row sums of the backward pass (up to two rows and two weights per slot)
constexpr int V2_GROUP = 128;          // slot positions per wave of the score pass

// The lane's four columns c0 + 4 lane + q: one 16-byte load (VEC) or four 4-byte loads; a column past the end loads 0.
template <bool VEC>
__device__ __forceinline__ void v2_load(const float *__restrict__ row, const int HC, const int c0, const int lane, float (&r)[4]) {
    if constexpr (VEC) {
        full_load4<true>(row, HC, c0, lane, r);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = c0 + 4 * lane + q;
            r[q] = c < HC ? row[c] : 0.f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void v2_store(float *__restrict__ row, const int HC, const int c0, const int lane, const float (&r)[4]) {
    if constexpr (VEC) {
        full_store4<true>(row, HC, c0, lane, r);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = c0 + 4 * lane + q;
            if (c < HC) row[c] = r[q];
        }
    }
}

// The heads of the lane's columns (-1: past the end) and the fold mask of the slab at c0: bit 6 q + s says that at step d = 1 << s
// plane q of this lane adds the value of lane + d.  ONE_HEAD: plane 0 alone, the head of the lane's first column.
// IN_LOOP (the many-slab form calls this per slab): the lane number is taken through an opaque copy, so that the compares below are made
// where they are used instead of being kept, one lane mask in scalar registers each, across the whole slot loop.
__device__ __forceinline__ int v2_here(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

__device__ __forceinline__ int v2_in_vgpr(int x) {
    asm("" : "+v"(x));
    return x;
}

template <bool ONE_HEAD, bool IN_LOOP = false>
__device__ __forceinline__ unsigned v2_fold_mask(const int c0, const int lane_, const int HC, const int C, int (&hd)[4]) {
    constexpr int PLANES = ONE_HEAD ? 1 : 4;
    const int lane = IN_LOOP ? v2_here(lane_) : lane_;
    unsigned m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = c0 + 4 * lane + q;
        hd[q] = q < PLANES ? (c < HC ? c / C : -1) : hd[0];
    }
#pragma unroll
    for (int q = 0; q < PLANES; ++q)
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const int other = __shfl_down(hd[q], 1 << s);
            if (lane + (1 << s) < 64 && hd[q] >= 0 && other == hd[q]) m |= 1u << (6 * q + s);
        }
    return m;
}

struct V2SlotArgs {
    const int *rowptr, *col;
    int N, nnz, H, C, HC;
    const float *rows;                   // [N, HC] gathered by col[p]: hl
    const float *own;                    // [N, HC] held per destination row: hr (scores) or g (DOT)
    const float *att;                    // [HC] (scores)
    float slope;
    int self_loops;
    float *e, *e_self;                   // [nnz, H], [N, H]
};

// Every product and every sum below is rounded on its own (include/graphpope_hip.h: the summation contract), so no contraction.
#pragma clang fp contract(off)

// top bit of `bit` set: a, else b -- as a bit select on the lanes' own registers (a compare per fold step would hold a lane mask in
// scalar registers for each of the 6 or 24 steps across the whole slot loop).
__device__ __forceinline__ float v2_pick(const unsigned bit, const float a, const float b) {
    unsigned all = (unsigned)((int)bit >> 31);
    asm("" : "+v"(all));                                             // (opaque: or the compiler turns the bit select back into a compare)
    return __uint_as_float((__float_as_uint(a) & all) | (__float_as_uint(b) & ~all));
}

__device__ __forceinline__ float v2_leaky(const float z, const float slope) { return z > 0.f ? z : slope * z; }

// The scores of the slots t = 0 .. cnt - 1 (cnt <= 64) of destination row v whose source ids lie in the lanes (`mine`: -1 = no term, the
// slot gets 0) into out[t * H + k].  SINGLE: H C <= 256, one slab, and att / the mask / the heads are the caller's registers (at1, m1,
// hd1); otherwise they are formed per slab.
template <bool VEC, bool ONE_HEAD, bool DOT, bool SINGLE>
__device__ __forceinline__ void v2_score_slots(const V2SlotArgs &a, const int v, int mine, const int cnt, float *out, const int lane,
                                               const float (&at1)[4], const unsigned m1, const int (&hd1)[4]) {
    constexpr int PLANES = ONE_HEAD ? 1 : 4, AHEAD = v2_ahead(ONE_HEAD, SINGLE);
    // the rarer forms keep the sizes in vector registers: their index arithmetic as scalar values, beside the four planes' or the slab
    // loop's own state, is more than the scalar registers hold
    constexpr bool RARE = !(ONE_HEAD && SINGLE);
    const int HC = RARE ? v2_in_vgpr(a.HC) : a.HC, H = RARE ? v2_in_vgpr(a.H) : a.H, C = RARE ? v2_in_vgpr(a.C) : a.C;
    const int slabs = SINGLE ? 1 : (a.HC + 255) / 256;
    const bool ok = mine >= 0;
    if (!ok) mine = 0;
    const unsigned long long live = __ballot(ok);
    for (int t0 = 0; t0 < cnt; t0 += AHEAD) {
        if ((live >> t0 & ((1ull << AHEAD) - 1)) == 0) {                               // no term among them (self-loop slots, bad ids)
            for (int u = 0; u < AHEAD && t0 + u < cnt; ++u)
                for (int k = lane; k < H; k += 64) out[(size_t)(t0 + u) * H + k] = 0.f;
            continue;
        }
        float carry[AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) carry[u] = 0.f;
        for (int s = 0; s < slabs; ++s) {
            const int c0 = s * 256;
            float r[AHEAD][4];
#pragma unroll
            for (int u = 0; u < AHEAD; ++u)                           // past the end: the last slot again, never stored
                v2_load<VEC>(a.rows + (size_t)__shfl(mine, min(t0 + u, cnt - 1)) * HC, HC, c0, lane, r[u]);
            float own[4], at[4];
            int hd[4];
            unsigned m;
            v2_load<VEC>(a.own + (size_t)v * HC, HC, c0, lane, own);
            if constexpr (SINGLE) {
#pragma unroll
                for (int q = 0; q < 4; ++q) { at[q] = at1[q]; hd[q] = hd1[q]; }
                m = m1;
            } else {
                if constexpr (!DOT) v2_load<VEC>(a.att, HC, c0, lane, at);
                m = v2_fold_mask<ONE_HEAD, true>(c0, lane, HC, C, hd);
            }
            // the terms, then the fold of every plane
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if constexpr (DOT) {
                        r[u][q] = own[q] * r[u][q];
                    } else {
                        const float z = r[u][q] + own[q];
                        r[u][q] = at[q] * v2_leaky(z, a.slope);
                    }
                }
                if constexpr (ONE_HEAD) {
                    const float s01 = r[u][0] + r[u][1];
                    const float s012 = s01 + r[u][2];
                    r[u][0] = s012 + r[u][3];
                }
#pragma unroll
                for (int q = 0; q < PLANES; ++q)
#pragma unroll
                    for (int st = 0; st < 6; ++st) {
                        const float sum = r[u][q] + __shfl_down(r[u][q], 1 << st);
                        r[u][q] = v2_pick(m << (31 - (6 * q + st)), sum, r[u][q]);
                    }
            }
            const int c_end = min(HC, c0 + 256);
            const int h_first = c0 / C, h_last = (c_end - 1) / C;
            const bool from_prev = !SINGLE && h_first * C < c0, goes_on = !SINGLE && (h_last + 1) * C > c0 + 256;
            if constexpr (ONE_HEAD) {
                const bool start = hd[0] >= 0 && (lane == 0 || hd[0] * C > c0 + 4 * lane - 4);             // the lane before lies in another head
                const int last_start = (max(h_last * C, c0) - c0) >> 2;
#pragma unroll
                for (int u = 0; u < AHEAD; ++u) {
                    float val = r[u][0];
                    if (from_prev && lane == 0) val = carry[u] + val;
                    if (goes_on) carry[u] = __shfl(val, last_start);
                    if (t0 + u < cnt && start && (hd[0] + 1) * C <= c0 + 256)
                        out[(size_t)(t0 + u) * H + hd[0]] = (live >> (t0 + u) & 1ull) ? val : 0.f;
                }
            } else {
                for (int base = h_first; base <= h_last; base += 64) {
                    const int h = base + v2_here(lane);                     // (opaque: the masks below live for this round only)
                    const bool valid = h <= h_last;
                    const int hh = min(h, h_last);
                    const int lo = max(hh * C, c0), hi = min((hh + 1) * C, c_end);
                    int from[4];
                    unsigned has[4];                                         // top bit: plane q has a column of the head
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c1 = lo + ((q - lo) & 3);                  // the head's first column in plane q
                        has[q] = valid && c1 < hi ? 0x80000000u : 0u;
                        from[q] = has[q] ? (c1 - c0) >> 2 : 0;
                    }
                    const bool last_round = base + 64 > h_last;
#pragma unroll
                    for (int u = 0; u < AHEAD; ++u) {
                        float part[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            part[q] = v2_pick(has[q], __shfl(r[u][q], from[q]), 0.f);
                        }
                        const float s01 = part[0] + part[1];
                        const float s012 = s01 + part[2];
                        float val = s012 + part[3];
                        if (from_prev && h == h_first) val = carry[u] + val;
                        if (goes_on && last_round) carry[u] = __shfl(val, h_last - base);
                        if (t0 + u < cnt && valid && (h + 1) * C <= c0 + 256)
                            out[(size_t)(t0 + u) * H + h] = (live >> (t0 + u) & 1ull) ? val : 0.f;
                    }
                }
            }
        }
    }
}

// One wave per work item: a run of V2_GROUP slot positions, or (behind them) the self term of one row.  Either is cut into chunks of at
// most 64 slots of ONE destination row, and every chunk takes the same call.
template <bool VEC, bool ONE_HEAD, bool DOT, bool SINGLE>
__global__ __launch_bounds__(256) void k_gatv2_scores(const V2SlotArgs a) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int N = a.N, nnz = a.nnz, H = a.H;
    const unsigned groups = ((unsigned)nnz + V2_GROUP - 1) / V2_GROUP, items = groups + (unsigned)N;    // < 2^31 / 128 + 2^31
    float at1[4] = {};
    int hd1[4] = {};
    unsigned m1 = 0;
    if constexpr (SINGLE) {
        if constexpr (!DOT) v2_load<VEC>(a.att, a.HC, 0, lane, at1);
        m1 = v2_fold_mask<ONE_HEAD>(0, lane, a.HC, a.C, hd1);
    }
    for (unsigned w = wave; w < items; w += min(nwaves, items - w)) {                                    // (no wrap-around behind the last item)
        const bool self = w >= groups;
        int v, p, P1;
        if (self) {
            v = (int)(w - groups); p = 0; P1 = 1;
        } else {
            p = (int)(w * V2_GROUP); P1 = min(nnz, p + V2_GROUP);
            int lo = 0, hi = N - 1;                                    // the row of slot p: the first whose (clamped) end lies behind it
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (min(max(a.rowptr[mid + 1], 0), nnz) > p) hi = mid; else lo = mid + 1;
            }
            v = lo;
        }
        while (p < P1) {
            int cnt, mine;
            float *out;
            if (self) {                                                // one term, v -> v; without self loops no term: e_self = 0
                cnt = 1; mine = lane == 0 && a.self_loops ? v : -1; out = a.e_self + (size_t)v * H; p = P1;
            } else {
                int beg, end;
                gat_row_bounds(a.rowptr, nnz, v, beg, end);
                if (end <= p) {
                    if (v < N - 1) { ++v; continue; }
                    for (long long t = (long long)p * H + lane; t < (long long)P1 * H; t += 64) a.e[t] = 0.f;   // slots behind the last row: no terms
                    break;
                }
                cnt = min(64, min(end, P1) - p);
                mine = lane < cnt ? a.col[p + lane] : -1;
                if ((unsigned)mine >= (unsigned)N || (a.self_loops && mine == v)) mine = -1;
                out = a.e + (size_t)p * H; p += cnt;
            }
            v2_score_slots<VEC, ONE_HEAD, DOT, SINGLE>(a, v, mine, cnt, out, lane, at1, m1, hd1);
        }
    }
}

struct V2SoftArgs {
    const int *rowptr, *col;
    int N, nnz, H;
    int self_loops;
    const float *e, *e_self;             // [nnz, H], [N, H]
    float *alpha, *alpha_self;           // may be e and e_self themselves
};

// One wave per (row i, head k) over a given e: k_gat_attention's order.  m = the largest e of the row's terms (exact); s: lane l adds
// exp(e - m) of the slots beg + l, beg + l + 64, .. ascending from +0, the 64 lane sums fold by the butterfly, then + the self term's
// exponential; alpha = exp(e - m) / s.  Every other slot of the row gets 0.
__global__ __launch_bounds__(256) void k_gatv2_softmax(const V2SoftArgs a) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long items = (long long)a.N * a.H;
    const int H = a.H;
    for (long long w = wave; w < items; w += nwaves) {
        const int v = (int)(w / H), k = (int)(w - (long long)v * H);
        int beg, end;
        gat_row_bounds(a.rowptr, a.nnz, v, beg, end);
        const float es = a.self_loops ? a.e_self[w] : -INFINITY;
        float m = es;
        for (int p = beg + lane; p < end; p += 64) {
            const int j = a.col[p];
            if ((unsigned)j < (unsigned)a.N && !(a.self_loops && j == v)) m = fmaxf(m, a.e[(size_t)p * H + k]);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
        float s = 0.f;
        for (int p = beg + lane; p < end; p += 64) {
            const int j = a.col[p];
            if ((unsigned)j < (unsigned)a.N && !(a.self_loops && j == v)) s = s + expf(a.e[(size_t)p * H + k] - m);
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
            if ((unsigned)j < (unsigned)a.N && !(a.self_loops && j == v)) al = expf(a.e[(size_t)p * H + k] - m) / s;
            a.alpha[(size_t)p * H + k] = al;
        }
        if (lane == 0) a.alpha_self[w] = a.self_loops ? xs / s : 0.f;
    }
}

// One wave per (row i, head k), one lane per slot over [nnz, H] scalars: de holds dalpha on entry.  t = sum alpha_p dalpha_p (lane sums
// ascending, the butterfly, then the self term); de_p = alpha_p (dalpha_p - t) in place (0 for a slot that is no term), de_self likewise.
__global__ __launch_bounds__(256) void k_gatv2_edge_grad(const int *__restrict__ rowptr, const int *__restrict__ col, const int N, const int nnz,
                                                         const int H, const int self_loops, const float *__restrict__ alpha,
                                                         const float *__restrict__ alpha_self, float *__restrict__ de, float *__restrict__ de_self) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long items = (long long)N * H;
    for (long long w = wave; w < items; w += nwaves) {
        const int v = (int)(w / H), k = (int)(w - (long long)v * H);
        int beg, end;
        gat_row_bounds(rowptr, nnz, v, beg, end);
        float t = 0.f;
        for (int p = beg + lane; p < end; p += 64) {
            const int j = col[p];
            if ((unsigned)j < (unsigned)N && !(self_loops && j == v)) {
                const float term = alpha[(size_t)p * H + k] * de[(size_t)p * H + k];
                t = t + term;
            }
        }
        t = gat_wave_sum(t);
        float ds = 0.f, as = 0.f;
        if (self_loops) {
            ds = de_self[w];
            as = alpha_self[w];
            const float term = as * ds;
            t = t + term;
        }
        for (int p = beg + lane; p < end; p += 64) {
            const int j = col[p];
            float x = 0.f;
            if ((unsigned)j < (unsigned)N && !(self_loops && j == v)) {
                const float dd = de[(size_t)p * H + k] - t;
                x = alpha[(size_t)p * H + k] * dd;
            }
            de[(size_t)p * H + k] = x;
        }
        if (lane == 0) {
            const float dd = ds - t;
            de_self[w] = self_loops ? as * dd : 0.f;
        }
    }
}

// ---- the row sums of the backward pass ----
// SRC = false, over the CSR by destination, row i:   grad_hr[i, c]  = sum over the row's terms of (de[p, k] att[c]) * leaky'(z)
//                                                    att_rows[i, c] = sum over the row's terms of  de[p, k] * leaky(z),   z = hl[j, c] + hr[i, c]
// SRC = true, over the CSR by source, row j:         grad_hl[j, c]  = sum over the out-edges of (de[p, k] att[c]) * leaky'(z), + alpha[p, k] * g[i, c]
//                                                    (p = slot_map[q], z = hl[j, c] + hr[i, c]: the same float sum as in the forward pass)
// Order: acc = +0, the slots ascending (per slot: + the de product, then + the alpha product), hub rows in runs of FULL_CHUNK slot
// positions added in run order, then the self term.  leaky'(z) = z > 0 ? 1 : slope.
struct V2RowArgs {
    const int *rowptr, *col;
    const int *slot_map;                 // SRC: [nnz] the slot of de / alpha that slot q reads
    int N, nnz, H, C, HC;
    const float *hl, *hr, *att;
    float slope;
    int self_loops;
    const float *de, *de_self;           // [nnz, H], [N, H]
    const float *alpha, *alpha_self;     // SRC
    const float *g;                      // SRC: [N, HC]
    float *out;                          // [N, HC]: grad_hr, or grad_hl
    float *out2;                         // SRC = false: att_rows [N, HC]
    int *counters, *hubs, *chunks;       // gcn.h's hub list
    float *partial;                      // [chunk_cap, 2 HC] (the second half: att_rows' runs)
    int hub_cap, chunk_cap;
};

template <bool SRC>
__device__ __forceinline__ void v2_row_term(const V2RowArgs &a, const float (&held)[4], const float (&at)[4], const float (&r)[4],
                                            const float (&gq)[4], const float (&wd)[4], const float (&wa)[4], float (&acc)[2][4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float z = SRC ? held[q] + r[q] : r[q] + held[q];           // hl + hr
        const bool on = z > 0.f;
        float dz = wd[q] * at[q];
        dz = dz * (on ? 1.0f : a.slope);
        acc[0][q] = acc[0][q] + dz;
        if constexpr (SRC) {
            const float t2 = wa[q] * gq[q];
            acc[0][q] = acc[0][q] + t2;
        } else {
            const float t2 = wd[q] * (on ? z : a.slope * z);
            acc[1][q] = acc[1][q] + t2;
        }
    }
}

template <bool VEC, bool SRC>
__device__ __forceinline__ void v2_row_add(const V2RowArgs &a, const int v, const int beg, const int end, const int c0, const int lane,
                                           const int (&hd)[4], const bool one_head, const float (&held)[4], const float (&at)[4],
                                           float (&acc)[2][4]) {
    const int HC = a.HC, H = a.H;
    for (int p0 = beg; p0 < end; p0 += 64) {
        const int p = p0 + lane;
        int mine = p < end ? a.col[p] : -1;
        int slot = p < end ? (SRC ? a.slot_map[p] : p) : -1;
        const bool ok = (unsigned)mine < (unsigned)a.N && (unsigned)slot < (unsigned)a.nnz && !(a.self_loops && mine == v);
        if (!ok) { mine = 0; slot = 0; }
        const unsigned long long live = __ballot(ok);
        const int cnt = min(64, end - p0);
        for (int t0 = 0; t0 < cnt; t0 += V2_ROW_AHEAD) {
            float r[V2_ROW_AHEAD][4], gq[V2_ROW_AHEAD][4], wd[V2_ROW_AHEAD][4], wa[V2_ROW_AHEAD][4];
#pragma unroll
            for (int u = 0; u < V2_ROW_AHEAD; ++u) {                     // past the end: the last slot again, loaded and not added
                const int t = min(t0 + u, cnt - 1);
                const size_t id = (size_t)__shfl(mine, t), sl = (size_t)__shfl(slot, t);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = one_head ? hd[0] : hd[q];
                    wd[u][q] = a.de[sl * H + k];
                    wa[u][q] = SRC ? a.alpha[sl * H + k] : 0.f;
                }
                v2_load<VEC>((SRC ? a.hr : a.hl) + id * HC, HC, c0, lane, r[u]);
                if constexpr (SRC) v2_load<VEC>(a.g + id * HC, HC, c0, lane, gq[u]);
            }
#pragma unroll
            for (int u = 0; u < V2_ROW_AHEAD; ++u)
                if (t0 + u < cnt && (live >> (t0 + u) & 1ull)) v2_row_term<SRC>(a, held, at, r[u], gq[u], wd[u], wa[u], acc);
        }
    }
}

template <bool VEC, bool SRC>
__device__ __forceinline__ void v2_row_finish(const V2RowArgs &a, const int v, const int c0, const int lane, const int (&hd)[4],
                                              const float (&held)[4], const float (&at)[4], float (&acc)[2][4]) {
    const int HC = a.HC, H = a.H;
    if (a.self_loops) {
        float r[4], gq[4] = {}, wd[4], wa[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            wd[q] = a.de_self[(size_t)v * H + hd[q]];
            wa[q] = SRC ? a.alpha_self[(size_t)v * H + hd[q]] : 0.f;
        }
        v2_load<VEC>((SRC ? a.hr : a.hl) + (size_t)v * HC, HC, c0, lane, r);
        if constexpr (SRC) v2_load<VEC>(a.g + (size_t)v * HC, HC, c0, lane, gq);
        v2_row_term<SRC>(a, held, at, r, gq, wd, wa, acc);
    }
    v2_store<VEC>(a.out + (size_t)v * HC, HC, c0, lane, acc[0]);
    if constexpr (!SRC) v2_store<VEC>(a.out2 + (size_t)v * HC, HC, c0, lane, acc[1]);
}

// The heads of the lane's columns for the weight loads (a column past the end counts as the last: loaded as 0, never stored).
__device__ __forceinline__ void v2_row_heads(const V2RowArgs &a, const int c0, const int lane, int (&hd)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) hd[q] = min(c0 + 4 * lane + q, a.HC - 1) / a.C;
}

template <bool VEC, bool SRC>
__global__ __launch_bounds__(256) void k_gatv2_rowsum(const V2RowArgs a, const bool one_head) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int HC = a.HC, slabs = (HC + 255) / 256;
    const int rows_stride = nwaves / slabs;
    const int slab = wave % slabs, first = wave / slabs;
    if (first >= rows_stride) return;
    const int c0 = slab * 256;
    int hd[4];
    v2_row_heads(a, c0, lane, hd);
    float at[4];
    v2_load<VEC>(a.att, HC, c0, lane, at);
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
        float held[4], acc[2][4] = {};
        v2_load<VEC>((SRC ? a.hl : a.hr) + (size_t)v * HC, HC, c0, lane, held);
        v2_row_add<VEC, SRC>(a, v, beg, end, c0, lane, hd, one_head, held, at, acc);
        v2_row_finish<VEC, SRC>(a, v, c0, lane, hd, held, at, acc);
    }
}

template <bool VEC, bool SRC>
__global__ __launch_bounds__(256) void k_gatv2_hub_partial(const V2RowArgs a, const bool one_head) {
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
        int hd[4];
        v2_row_heads(a, c0, lane, hd);
        float at[4], held[4], acc[2][4] = {};
        v2_load<VEC>(a.att, HC, c0, lane, at);
        v2_load<VEC>((SRC ? a.hl : a.hr) + (size_t)v * HC, HC, c0, lane, held);
        v2_row_add<VEC, SRC>(a, v, beg, end, c0, lane, hd, one_head, held, at, acc);
        v2_store<VEC>(a.partial + (size_t)e * 2 * HC, HC, c0, lane, acc[0]);
        if constexpr (!SRC) v2_store<VEC>(a.partial + (size_t)e * 2 * HC + HC, HC, c0, lane, acc[1]);
    }
}

template <bool VEC, bool SRC>
__global__ __launch_bounds__(256) void k_gatv2_hub_finish(const V2RowArgs a) {
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
        float acc[2][4] = {};
        for (int k = 0; k < nch; ++k) {                              // the runs' partial rows, added in run order
            float part[4];
            v2_load<VEC>(a.partial + (size_t)(base + k) * 2 * HC, HC, c0, lane, part);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[0][q] = acc[0][q] + part[q];
            if constexpr (!SRC) {
                v2_load<VEC>(a.partial + (size_t)(base + k) * 2 * HC + HC, HC, c0, lane, part);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[1][q] = acc[1][q] + part[q];
            }
        }
        int hd[4];
        v2_row_heads(a, c0, lane, hd);
        float at[4], held[4];
        v2_load<VEC>(a.att, HC, c0, lane, at);
        v2_load<VEC>((SRC ? a.hl : a.hr) + (size_t)v * HC, HC, c0, lane, held);
        v2_row_finish<VEC, SRC>(a, v, c0, lane, hd, held, at, acc);
    }
}

// Shared weights: a[i] = a[i] + b[i].
__global__ __launch_bounds__(256) void k_gatv2_add(float *__restrict__ a, const float *__restrict__ b, const long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) a[i] = a[i] + b[i];
}
#pragma clang fp contract(fast)

// ---- where everything lies in the scratch buffers: laid out HERE and nowhere else (offsets are multiples of 256, a function of the sizes) ----
//   forward:    gat.h's propagate layout (agg [N, HC] with concat = false | the hub region at width HC)
//   backward:   de [nnz, H] | de_self [N, H] | g [N, HC] (concat = false only) | GL, GR, AR [N, HC] each | slab [splits, HC, c_in] |
//               colsum [COLSUM_SPLITS, HC] | the hub region at width 2 HC
struct V2Scratch {
    size_t de, de_self, g, GL, GR, AR, slab, colsum, total;
    GcnHubScratch hub;
};

static bool v2_shape_ok(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C) {
    return gat_shape_ok(N, nnz, c_in, H, C) && (int64_t)H * C <= INT32_MAX / 4;
}

static V2Scratch v2_backward_scratch(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, bool concat) {
    V2Scratch s{};
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t was = at; at += align_up(bytes, 256); return was; };
    const size_t HC = (size_t)H * C;
    s.de = take(std::max<size_t>((size_t)nnz, 1) * H * sizeof(float));
    s.de_self = take((size_t)N * H * sizeof(float));
    if (!concat) s.g = take((size_t)N * HC * sizeof(float));
    s.GL = take((size_t)N * HC * sizeof(float));
    s.GR = take((size_t)N * HC * sizeof(float));
    s.AR = take((size_t)N * HC * sizeof(float));
    s.slab = take((size_t)gcn_weight_splits(N, (int)HC, c_in) * HC * c_in * sizeof(float));
    s.colsum = take((size_t)COLSUM_SPLITS * HC * sizeof(float));
    s.hub = gcn_hub_scratch(take, nnz, (int32_t)(2 * HC));
    s.total = at;
    return s;
}

// ---- which kernels a call runs: decided HERE; the lists below launch or print what this says (no HIP calls) ----
struct V2Aligned { bool x, w_l, w_r, hl, hr, att, io, grad_x, scratch; };   // io: out (forward) / grad_out (backward)

struct V2Plan {
    bool share, concat;
    bool score_vec, one_head;              // the score pass: 16-byte loads; a lane's columns lie in one head (C % 4 == 0)
    GatPlan gat;                           // gat.h's plan of the same pass: the projection (per product) and the propagate, or the dense tail
    bool dot_vec, row_vec;                 // backward: dalpha's loads, the row sums' loads
    bool colsum_rows_vec;
};

// The score pass over hl, hr and att (pope_gatv2_scores, pope_gatv2_attention and the forward pass).
static void v2_score_plan(V2Plan &p, int32_t H, int32_t C, bool al_hl, bool al_hr, bool al_att) {
    p.one_head = (C & 3) == 0;
    p.score_vec = ((H * C) & 3) == 0 && al_hl && al_hr && al_att;
}

static V2Plan v2_forward_plan(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, bool concat, bool share, int cus, const V2Aligned &al) {
    V2Plan p{};
    p.share = share; p.concat = concat;
    v2_score_plan(p, H, C, al.hl, al.hr, al.att);
    p.gat = gat_forward_plan(N, nnz, c_in, H, C, concat, cus, GatAligned{al.x, al.w_l && al.w_r, al.hl && al.hr, al.io, true, al.scratch});
    return p;
}

// gat.h's backward plan with W_l (the hub launches, both weight gradients, grad_bias), and with two weights the second product of grad_x.
static V2Plan v2_backward_plan(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, bool concat, bool share, bool need_grad_x,
                               const V2Aligned &al) {
    V2Plan p{};
    const int M = (int)N, HC = H * C;
    p.share = share; p.concat = concat;
    p.one_head = (C & 3) == 0;
    const bool g_al = concat ? al.io : al.scratch;
    p.dot_vec = (HC & 3) == 0 && al.hl && g_al;
    p.row_vec = (HC & 3) == 0 && al.hl && al.hr && al.att && g_al && al.scratch;
    p.gat = gat_backward_plan(N, nnz, c_in, H, C, concat, need_grad_x, GatAligned{al.x, al.w_l, al.hl, al.io, al.grad_x, al.scratch});
    if (!share) {   // grad_x[r, i] = sum_o GL[r, o] W_l[o, i] + sum_o GR[r, o] W_r[o, i] in one launch: G depth-contiguous, W outer-contiguous
        const Layout g = pick_layout(al.scratch, HC, 1, M, HC);
        p.gat.x_layouts = gemm_layouts(g, pick_layout(al.w_l, 1, c_in, c_in, HC), true, g, pick_layout(al.w_r, 1, c_in, c_in, HC), false, LAYOUT_GENERIC);
    }
    p.colsum_rows_vec = (HC & 3) == 0 && al.scratch;
    return p;
}

// ---- the launches of each call, written ONCE: the entry points run these lists, pope_gatv2_kernel_name prints them (layer_host.h) ----
template <bool VEC, bool ONE_HEAD, bool DOT, bool SINGLE, class Sink>
static void v2_scores_launch(Sink &s, const V2SlotArgs &a) {
    const size_t items = ((size_t)a.nnz + V2_GROUP - 1) / V2_GROUP + (size_t)a.N;
    s.launch(KName{"k_gatv2_scores<%s, %s, %s, %s>", tf(VEC), tf(ONE_HEAD), tf(DOT), tf(SINGLE)}, k_gatv2_scores<VEC, ONE_HEAD, DOT, SINGLE>,
             dim3(capped_grid(items * 64, 256)), dim3(256), a);
}

template <bool DOT, bool SINGLE, class Sink>
static void v2_scores_as(Sink &s, const V2SlotArgs &a, bool vec, bool one_head) {
    if (vec && one_head) v2_scores_launch<true, true, DOT, SINGLE>(s, a);
    else if (vec) v2_scores_launch<true, false, DOT, SINGLE>(s, a);
    else if (one_head) v2_scores_launch<false, true, DOT, SINGLE>(s, a);
    else v2_scores_launch<false, false, DOT, SINGLE>(s, a);
}

// (the fourth template argument: H C <= 256, one slab)
template <bool DOT, class Sink>
static void v2_scores(Sink &s, const V2SlotArgs &a, bool vec, bool one_head) {
    if (a.HC <= 256) v2_scores_as<DOT, true>(s, a, vec, one_head);
    else v2_scores_as<DOT, false>(s, a, vec, one_head);
}

template <class Sink>
static void v2_softmax(Sink &s, const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, int32_t H, int self_loops, const float *e,
                       const float *e_self, float *alpha, float *alpha_self) {
    const V2SoftArgs a{rowptr, col, (int)N, (int)nnz, H, self_loops, e, e_self, alpha, alpha_self};
    s.launch(KName{"k_gatv2_softmax"}, k_gatv2_softmax, dim3(capped_grid((size_t)N * H * 64, 256)), dim3(256), a);
}

template <bool VEC, bool SRC, class Sink>
static void v2_rowsum_as(Sink &s, const V2RowArgs &a, bool hubs, bool one_head) {
    hub_family(s, hubs, k_gcn_clear, a, a.HC, KName{"k_gatv2_rowsum<%s, %s>", tf(VEC), tf(SRC)}, k_gatv2_rowsum<VEC, SRC>,
               KName{"k_gatv2_hub_partial<%s, %s>", tf(VEC), tf(SRC)}, k_gatv2_hub_partial<VEC, SRC>,
               KName{"k_gatv2_hub_finish<%s, %s>", tf(VEC), tf(SRC)}, k_gatv2_hub_finish<VEC, SRC>, one_head);
}

template <bool SRC, class Sink>
static void v2_rowsum(Sink &s, V2RowArgs a, const GcnHubScratch &lay, const V2Plan &plan) {
    hub_bind(a, s, lay);
    if (plan.row_vec) v2_rowsum_as<true, SRC>(s, a, plan.gat.hubs, plan.one_head);
    else v2_rowsum_as<false, SRC>(s, a, plan.gat.hubs, plan.one_head);
}

// plan.share: hr is not written and hl serves as both.
template <class Sink>
static void v2_forward(Sink &s, const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *x, int32_t c_in, const float *weight_l,
                       const float *bias_l, const float *weight_r, const float *bias_r, const float *att, const float *bias, int32_t H, int32_t C,
                       float slope, int self_loops, float *hl, float *hr, float *alpha, float *alpha_self, float *out, const GatScratch &lay,
                       const V2Plan &plan) {
    const int HC = H * C;
    for (int side = 0; side < (plan.share ? 1 : 2); ++side)
        project(s, x, c_in, (int)N, HC, Operand{side ? weight_r : weight_l, c_in, 1}, side ? bias_r : bias_l, side ? hr : hl, plan.gat.rb, plan.gat.p_tile,
                plan.gat.p_layouts);
    const V2SlotArgs a{rowptr, col, (int)N, (int)nnz, H, C, HC, hl, plan.share ? hl : hr, att, slope, self_loops, alpha, alpha_self};
    v2_scores<false>(s, a, plan.score_vec, plan.one_head);
    v2_softmax(s, rowptr, col, N, nnz, H, self_loops, alpha, alpha_self, alpha, alpha_self);
    gat_aggregate(s, rowptr, col, N, nnz, alpha, self_loops ? alpha_self : nullptr, hl, H, C, bias, out, lay, plan.gat);
}

// plan.share: hr, grad_weight_r and grad_bias_r are not used.  want_bias_l, _r, want_bias: that bias gradient is asked for (the query: every one).
template <class Sink>
static void v2_backward(Sink &s, const int32_t *rowptr, const int32_t *col, const int32_t *rowptr_t, const int32_t *col_t, const int32_t *slot_map,
                        int64_t N, int64_t nnz, const float *x, int32_t c_in, const float *weight_l, const float *weight_r, const float *att, int32_t H,
                        int32_t C, float slope, int self_loops, const float *hl, const float *hr, const float *alpha, const float *alpha_self,
                        const float *grad_out, float *grad_x, float *grad_weight_l, bool want_bias_l, float *grad_bias_l, float *grad_weight_r,
                        bool want_bias_r, float *grad_bias_r, float *grad_att, bool want_bias, float *grad_bias, const V2Scratch &lay,
                        const V2Plan &plan) {
    const int HC = H * C;
    const bool share = plan.share;
    float *de = s.floats(lay.de), *de_self = s.floats(lay.de_self), *GL = s.floats(lay.GL), *GR = s.floats(lay.GR), *AR = s.floats(lay.AR);
    float *colsum = s.floats(lay.colsum);
    const float *g = gat_spread_grad(s, plan.concat, grad_out, N, H, C, lay.g);
    const V2SlotArgs da{rowptr, col, (int)N, (int)nnz, H, C, HC, hl, g, nullptr, slope, self_loops, de, de_self};
    v2_scores<true>(s, da, plan.dot_vec, plan.one_head);
    s.launch(KName{"k_gatv2_edge_grad"}, k_gatv2_edge_grad, dim3(capped_grid((size_t)N * H * 64, 256)), dim3(256), rowptr, col, (int)N, (int)nnz, H,
             self_loops, alpha, alpha_self, de, de_self);
    V2RowArgs ra{};
    ra.N = (int)N; ra.nnz = (int)nnz; ra.H = H; ra.C = C; ra.HC = HC;
    ra.hl = hl; ra.hr = share ? hl : hr; ra.att = att; ra.slope = slope; ra.self_loops = self_loops;
    ra.de = de; ra.de_self = de_self;
    V2RowArgs dst = ra;
    dst.rowptr = rowptr; dst.col = col; dst.out = GR; dst.out2 = AR;
    v2_rowsum<false>(s, dst, lay.hub, plan);
    V2RowArgs src = ra;
    src.rowptr = rowptr_t; src.col = col_t; src.slot_map = slot_map; src.alpha = alpha; src.alpha_self = alpha_self; src.g = g; src.out = GL;
    v2_rowsum<true>(s, src, lay.hub, plan);
    s.colsum(AR, (int)N, HC, colsum, plan.colsum_rows_vec, grad_att);
    if (share) s.launch(KName{"k_gatv2_add"}, k_gatv2_add, dim3(capped_grid((size_t)N * HC, 256)), dim3(256), GL, GR, (long long)N * HC);
    for (int side = 0; side < (share ? 1 : 2); ++side) {
        float *G = side ? GR : GL;
        split_depth_gemm(s, G, HC, x, c_in, (int)N, side ? grad_weight_r : grad_weight_l, plan.gat.splits, s.floats(lay.slab), plan.gat.w_tile,
                         plan.gat.w_layouts);
        if (side ? want_bias_r : want_bias_l) s.colsum(G, (int)N, HC, colsum, plan.colsum_rows_vec, side ? grad_bias_r : grad_bias_l);
    }
    if (plan.gat.need_grad_x) {
        GemmArgs px = gemm_problem(Operand{GL, HC, 1}, Operand{weight_l, 1, c_in}, HC, (int)N, c_in, grad_x, c_in);
        if (!share) { px.A1 = Operand{GR, HC, 1}; px.B1 = Operand{weight_r, 1, c_in}; px.K1 = HC; }
        s.gemm(px, plan.gat.x_tile, plan.gat.x_layouts);
    }
    if (want_bias) s.colsum(grad_out, (int)N, plan.concat ? HC : C, colsum, plan.gat.colsum_vec, grad_bias);
}

static const char *const V2_SIZE_MSG = "bad size (N in (0, INT32_MAX), nnz in [0, INT32_MAX), c_in, H, C > 0, H C <= INT32_MAX / 4)";

}  // namespace pope

using namespace pope;

// The score pass, and with alpha the edge softmax behind it (pope_gatv2_scores / pope_gatv2_attention as `who`, their pointers checked).
static int v2_scores_entry(const char *who, const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *hl, const float *hr,
                           int32_t H, int32_t C, const float *att, float slope, int self_loops, float *e, float *e_self, float *alpha,
                           float *alpha_self, void *stream) {
    POPE_REQUIRE(v2_shape_ok(N, nnz, 1, H, C), "%s: %s", who, V2_SIZE_MSG);
    POPE_REQUIRE(gat_slope_ok(slope), "%s: negative_slope must be in [0, 1]", who);
    const V2SlotArgs a{rowptr, col, (int)N, (int)nnz, H, C, H * C, hl, hr, att, slope, self_loops, e, e_self};
    V2Plan plan{};
    v2_score_plan(plan, H, C, aligned16(hl), aligned16(hr), aligned16(att));
    LaunchRun run{nullptr, (hipStream_t)stream, 0};
    v2_scores<false>(run, a, plan.score_vec, plan.one_head);
    if (alpha_self) v2_softmax(run, rowptr, col, N, nnz, H, self_loops, e, e_self, alpha, alpha_self);
    return run.done();
}

// e [nnz, H] and e_self [N, H] (0 for a slot that is no term; e_self 0 without self loops).  The order of every e: the head of this file.
extern "C" int pope_gatv2_scores(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *hl, const float *hr, int32_t H,
                                 int32_t C, const float *att, float negative_slope, int32_t add_self_loops, float *e, float *e_self, void *stream) {
    clear_error();
    POPE_REQUIRE(rowptr && ((col && e) || nnz == 0) && hl && hr && att && e_self, "pope_gatv2_scores: null pointer");
    return v2_scores_entry("pope_gatv2_scores", rowptr, col, N, nnz, hl, hr, H, C, att, negative_slope, add_self_loops != 0, e, e_self, nullptr, nullptr, stream);
}

// The scores as above, then the edge softmax over them: lane sums ascending, the xor butterfly, then the self term; expf.
extern "C" int pope_gatv2_attention(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *hl, const float *hr, int32_t H,
                                    int32_t C, const float *att, float negative_slope, int32_t add_self_loops, float *e, float *e_self,
                                    float *alpha, float *alpha_self, void *stream) {
    clear_error();
    POPE_REQUIRE(rowptr && ((col && e && alpha) || nnz == 0) && hl && hr && att && e_self && alpha_self, "pope_gatv2_attention: null pointer");
    return v2_scores_entry("pope_gatv2_attention", rowptr, col, N, nnz, hl, hr, H, C, att, negative_slope, add_self_loops != 0, e, e_self, alpha, alpha_self,
                           stream);
}

extern "C" size_t pope_gatv2_conv_forward_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, int32_t concat) {
    return v2_shape_ok(N, nnz, c_in, H, C) ? gat_scratch(GAT_PROPAGATE, N, nnz, c_in, H, C, concat != 0).total : 0;
}

// weight_r NULL: shared weights, hr is not written and hl serves as both.  Order: the projections' (the GEMM kernels', + the linear bias
// last), e and the softmax as above (e lies in alpha until the softmax replaces it), then pope_gat_propagate's.
extern "C" int pope_gatv2_conv_forward(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *x, int32_t c_in,
                                       const float *weight_l, const float *bias_l, const float *weight_r, const float *bias_r, const float *att,
                                       const float *bias, int32_t H, int32_t C, int32_t concat, float negative_slope, int32_t add_self_loops,
                                       float *hl, float *hr, float *alpha, float *alpha_self, float *out, void *scratch, size_t scratch_bytes,
                                       void *stream_) {
    clear_error();
    const bool share = weight_r == nullptr;
    POPE_REQUIRE(rowptr && ((col && alpha) || nnz == 0) && x && weight_l && att && hl && (share || hr) && alpha_self && out && scratch,
                 "pope_gatv2_conv_forward: null pointer");
    POPE_REQUIRE(v2_shape_ok(N, nnz, c_in, H, C), "pope_gatv2_conv_forward: %s", V2_SIZE_MSG);
    POPE_REQUIRE(gat_slope_ok(negative_slope), "pope_gatv2_conv_forward: negative_slope must be in [0, 1]");
    POPE_REQUIRE(share || hr != hl, "pope_gatv2_conv_forward: hr must not alias hl");
    POPE_REQUIRE(out != hl && out != hr && out != alpha && out != alpha_self, "pope_gatv2_conv_forward: out must not alias hl, hr, alpha or alpha_self");
    const GatScratch lay = gat_scratch(GAT_PROPAGATE, N, nnz, c_in, H, C, concat != 0);
    if (scratch_bytes < lay.total) return scratch_too_small("pope_gatv2_conv_forward", scratch_bytes, lay.total);
    int cus = 0, rc;
    if ((rc = device_cu_count(&cus))) return rc;
    const V2Plan plan = v2_forward_plan(N, nnz, c_in, H, C, concat != 0, share, cus,
                                        V2Aligned{aligned16(x), aligned16(weight_l), share || aligned16(weight_r), aligned16(hl),
                                                  aligned16(share ? hl : hr), aligned16(att), aligned16(out), true, aligned16(scratch)});
    LaunchRun run{scratch, (hipStream_t)stream_, cus};
    v2_forward(run, rowptr, col, N, nnz, x, c_in, weight_l, bias_l, weight_r, bias_r, att, bias, H, C, negative_slope, add_self_loops != 0, hl, hr, alpha,
               alpha_self, out, lay, plan);
    return run.done();
}

extern "C" size_t pope_gatv2_conv_backward_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, int32_t concat) {
    return v2_shape_ok(N, nnz, c_in, H, C) ? v2_backward_scratch(N, nnz, c_in, H, C, concat != 0).total : 0;
}

// weight_r NULL: shared weights (hr, grad_weight_r and grad_bias_r are not used; grad_weight_l and grad_bias_l take the sum
// grad_hl + grad_hr, added element by element first).  Orders: dalpha as e; t and de: lane sums ascending, the butterfly, the self
// term; the row sums: slots ascending, hub runs in run order, the self term last; grad_att, the linear-bias gradients and grad_bias:
// k_colsum_partial's row slices, then the slices in order; the weight gradients and grad_x: the tile kernel's (depth splits in order;
// grad_x = grad_hl W_l, then + grad_hr W_r in the same accumulators).
extern "C" int pope_gatv2_conv_backward(const int32_t *rowptr, const int32_t *col, const int32_t *rowptr_t, const int32_t *col_t,
                                        const int32_t *slot_map, int64_t N, int64_t nnz, const float *x, int32_t c_in, const float *weight_l,
                                        const float *weight_r, const float *att, int32_t H, int32_t C, int32_t concat, float negative_slope,
                                        int32_t add_self_loops, const float *hl, const float *hr, const float *alpha, const float *alpha_self,
                                        const float *grad_out, float *grad_x, float *grad_weight_l, float *grad_bias_l, float *grad_weight_r,
                                        float *grad_bias_r, float *grad_att, float *grad_bias, void *scratch, size_t scratch_bytes, void *stream_) {
    clear_error();
    const bool share = weight_r == nullptr;
    POPE_REQUIRE(rowptr && rowptr_t && ((col && col_t && slot_map && alpha) || nnz == 0) && x && weight_l && att && hl && (share || (hr && grad_weight_r)) &&
                     alpha_self && grad_out && grad_weight_l && grad_att && scratch,
                 "pope_gatv2_conv_backward: null pointer");
    POPE_REQUIRE(v2_shape_ok(N, nnz, c_in, H, C), "pope_gatv2_conv_backward: %s", V2_SIZE_MSG);
    POPE_REQUIRE(gat_slope_ok(negative_slope), "pope_gatv2_conv_backward: negative_slope must be in [0, 1]");
    const bool cat = concat != 0;
    const V2Scratch lay = v2_backward_scratch(N, nnz, c_in, H, C, cat);
    if (scratch_bytes < lay.total) return scratch_too_small("pope_gatv2_conv_backward", scratch_bytes, lay.total);
    const V2Plan plan = v2_backward_plan(N, nnz, c_in, H, C, cat, share, grad_x != nullptr,
                                         V2Aligned{aligned16(x), aligned16(weight_l), share || aligned16(weight_r), aligned16(hl),
                                                   aligned16(share ? hl : hr), aligned16(att), aligned16(grad_out), aligned16(grad_x), aligned16(scratch)});
    LaunchRun run{scratch, (hipStream_t)stream_, 0};
    v2_backward(run, rowptr, col, rowptr_t, col_t, slot_map, N, nnz, x, c_in, weight_l, weight_r, att, H, C, negative_slope, add_self_loops != 0, hl, hr,
                alpha, alpha_self, grad_out, grad_x, grad_weight_l, grad_bias_l != nullptr, grad_bias_l, grad_weight_r, grad_bias_r != nullptr, grad_bias_r,
                grad_att, grad_bias != nullptr, grad_bias, lay, plan);
    return run.done();
}

// The launches of pope_gatv2_conv_forward (backward = 0) or pope_gatv2_conv_backward (backward != 0, with every bias gradient) for this
// shape on a device of cu_count CUs, in launch order: the lists above under the plan functions, printed.  Bit i of `misaligned`: operand i
// of {x, weight_l, weight_r, hl, hr, att, out or grad_out, grad_x, scratch} is not 16-byte aligned.
extern "C" int pope_gatv2_kernel_name(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, int32_t concat, int32_t share_weights,
                                      int32_t backward, int32_t need_grad_x, int32_t cu_count, uint32_t misaligned, char *name, size_t cap) {
    clear_error();
    POPE_REQUIRE(name && cap > 0 && v2_shape_ok(N, nnz, c_in, H, C) && cu_count > 0 && misaligned < (1u << 9), "pope_gatv2_kernel_name: bad argument");
    const auto ok = [misaligned](int bit) { return !(misaligned >> bit & 1u); };
    const bool cat = concat != 0, share = share_weights != 0;
    const V2Aligned al{ok(0), ok(1), share || ok(2), ok(3), share ? ok(3) : ok(4), ok(5), ok(6), ok(7), ok(8)};
    const V2Plan p = backward ? v2_backward_plan(N, nnz, c_in, H, C, cat, share, need_grad_x != 0, al)
                              : v2_forward_plan(N, nnz, c_in, H, C, cat, share, cu_count, al);
    LaunchNames names{cu_count};
    if (backward)
        v2_backward(names, nullptr, nullptr, nullptr, nullptr, nullptr, N, nnz, nullptr, c_in, nullptr, nullptr, nullptr, H, C, 0.f, 0, nullptr, nullptr,
                    nullptr, nullptr, nullptr, nullptr, nullptr, true, nullptr, nullptr, true, nullptr, nullptr, true, nullptr,
                    v2_backward_scratch(N, nnz, c_in, H, C, cat), p);
    else
        v2_forward(names, nullptr, nullptr, N, nnz, nullptr, c_in, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, H, C, 0.f, 0, nullptr, nullptr,
                   nullptr, nullptr, nullptr, gat_scratch(GAT_PROPAGATE, N, nnz, c_in, H, C, cat), p);
    return names.names.copy_to("pope_gatv2_kernel_name", name, cap);
}
