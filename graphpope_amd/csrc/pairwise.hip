// node2vec-space GraphPOPE embedding on MI355X (gfx950): N x K pairwise distance to the anchor rows as an
// exact-f32 MFMA tile, then per-column min-max scaling.
//
// Replaces /root/reference/utils.py:158-176 (sklearn cosine_similarity / cosine_distances / euclidean_distances
// followed by MinMaxScaler().fit/transform).  pairwise_plan (below: pure host logic) writes a call down as an ordered list of
// steps; pairwise_features_impl walks the list and launches, pope_pairwise_kernel_name walks it and prints.  Two pipelines
// (DESIGN.md §4), each with the feature copy out[:, :F] = x (utils.py:177 concat_into_features) where x is given:
//  (A) depth <= 128 in 16-byte pieces, out below 4 GB -- the node2vec table is [N, 128]:
//   PW_SIDE_FORK      the side stream waits for what the caller's stream holds (side_copy.hip)
//   PW_PERSISTENT     k_pairwise_persistent (pairwise_persistent.h): one block per CU, the anchor rows resident in LDS, the table
//                     streamed through by LDS-DMA; row norms, metric epilogue, raw values into out[:, c0:], per-block column min / max
//   PW_SIDE_COPY      k_copy_features: out[:, :F] = x on the side stream, beside that kernel
//   PW_MINMAX_FINISH  k_minmax_finish: column min / max over the partial rows -> scale_ = 1/range (range < 10 eps -> 1), min_ = 0 - min*scale_
//   PW_MINMAX_APPLY   k_minmax_apply / k_minmax_apply4: y = e * scale_ + min_ in place (two roundings, like NumPy's X *= scale_; X += min_)
//   PW_SIDE_JOIN      the caller's stream waits for the copy
//  (B) everything else -- round 1's pipeline:
//   PW_GATHER_ANCHOR_ROWS  k_gather_anchor_rows: anchors given as row ids become a matrix in the scratch buffer
//   PW_SQNORM         k_sqnorm: ||x||^2 of every node2vec row and anchor row, accumulated in f64, as {(float)|r|^2, 1/|r|}
//   PW_ONE_TILE       k_pairwise: dot(X, A^T) with v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulate; 64 x 128 tiles on the
//                     machinery of gemm_tile.h: register double buffering, batched LDS fragment reads), metric
//                     epilogue, raw values written straight into the [N, F+K] output, per-block column min/max.
//                     The blocks also carry the feature copy: each streams its own rows' share between its tile product and its epilogue.
//   PW_MINMAX_FOLD, PW_MINMAX_REDUCE   k_minmax_fold / k_minmax_reduce: column min/max over blocks (two stages), then PW_MINMAX_APPLY
//  and in front of either, PW_CONCAT: pope_concat as a pass of its own, for an x that neither copy can take.
// Measured and rejected (round 2): computing the tile TWICE (statistics pass, then a pass that scales in its epilogue and
// stores once) instead of raw store + apply pass: with kernel (B) two tile passes took 244 us against 161 us for tile +
// apply; with kernel (A), built and measured in round 4, 0.219 ms against 0.171 for the whole call: a second exact-f32 MFMA
// pass costs 58 us, the 182 MB scaling pass it removes 35 (profiles/r04_pairwise_two_pass.txt).
// Euclidean: sklearn upcasts f32 inputs to f64 (pairwise.py:582-653).  Here the row norms are accumulated in f64,
// d2 = xx + aa - 2 dot is one f32 fma on the f32-accumulated MFMA dot (whose own error, ~1e-6 |x||a|, dominates);
// where d2 < PW_CANCEL_RATIO (= 2^-3) of the norms (cancellation) the entry is recomputed as a direct sum of squared
// differences, so coincident rows give exactly 0 instead of ~1e-2 and rows that share an offset (d2 / norms ~
// sigma^2 / (mu^2 + sigma^2)) keep their digits (pairwise_epilogue.h: one epilogue for both tile kernels).  Gate: 1e-5 absolute
// on the scaled values against float64, anchors among the table rows (tests/test_pairwise_conditioning_gpu.py); the cosine
// metrics are held to scikit-learn's float32 result.
#include "pairwise_persistent.h"   // pairwise_epilogue.h, gemm_tile.h
#include "side_copy.h"

#include <cstring>

namespace pope {

constexpr int PM = 64, PN = 128, PWM = 2, PWN = 2;    // rows of X x anchor columns per block of k_pairwise: 4 waves as 2 x 2, each 32 x 64 (two MFMA tiles)

int g_pairwise_kernel = 0;             // pope_debug_set(POPE_KNOB_PAIRWISE_KERNEL, ...), declared in common.h: an input of pairwise_plan

// Sum of squares of every row in f64 (sklearn row_norms on the upcast chunk), handed to the tile kernels' epilogues the
// way they use it: {(float)|row|^2, 1 / |row|} with 1 for a zero row (sklearn normalize(): zero rows stay zero).
// VEC: rows of 16-byte pieces (D % 4 == 0, aligned base): 16 lanes per row, four rows per wave and step -- the [N, 128]
// table at 4-byte loads, one wave per row, read at 2 TB/s.
// One launch for both matrices: rows [0, rows) of m, then rows [0, rows2) of m2 (same depth).
template <bool VEC>
__global__ __launch_bounds__(256) void k_sqnorm(const float *__restrict__ m, long long rows, float2 *__restrict__ out,
                                                const float *__restrict__ m2, long long rows2, float2 *__restrict__ out2, int D) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long total = rows + rows2;
    if (VEC) {
        const int sub = lane & 15, D4 = D >> 2;
        for (long long r = wave * 4 + (lane >> 4); r < (total + 3) / 4 * 4; r += nwaves * 4) {
            const float *row = r < rows ? m + r * D : m2 + (r - rows) * D;
            double acc = 0.0;
            if (r < total)
                for (int k = sub; k < D4; k += 16) {
                    const f32x4v v = __builtin_nontemporal_load(reinterpret_cast<const f32x4v *>(row) + k);
                    acc += (double)v.x * (double)v.x;
                    acc += (double)v.y * (double)v.y;
                    acc += (double)v.z * (double)v.z;
                    acc += (double)v.w * (double)v.w;
                }
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
            if (sub == 0 && r < total) (r < rows ? out[r] : out2[r - rows]) = row_norm_pair(acc);
        }
        return;
    }
    for (long long r = wave; r < total; r += nwaves) {
        const float *row = r < rows ? m + r * D : m2 + (r - rows) * D;
        double acc = 0.0;
        for (int k = lane; k < D; k += 64) {
            const double v = (double)row[k];
            acc += v * v;
        }
        acc = wave_sum(acc);
        if (lane == 0) (r < rows ? out[r] : out2[r - rows]) = row_norm_pair(acc);
    }
}

// grid = (ceil(N / PM), ceil(K / PN)).  dot(X, A^T) on the shared MFMA tile machinery (gemm_tile.h), then the metric
// epilogue, the raw values into out[:, c0:], and this block's column min / max.
// The feature copy a pass carries: float4 columns [c_lo, c_hi) of x [N, F4 * 4] -> out[:, 0 : F4 * 4]; x == nullptr: none.
struct PwCopy {
    const float *x;
    int F4, c_lo, c_hi;
};

template <int LAYOUT>
__global__ __launch_bounds__(256) void k_pairwise(const float *__restrict__ X, int N, int D, const float *__restrict__ A,
                                                  int K, int metric, const float2 *__restrict__ xx, const float2 *__restrict__ aa,
                                                  float *__restrict__ out, long long out_cols, int c0,
                                                  float *__restrict__ part_min, float *__restrict__ part_max, int Kpad, PwCopy cp) {
    constexpr int NT = PN / PWN / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *As = reinterpret_cast<float *>(smem);
    float *Bs = As + Tile<PM>::FLOATS;
    __shared__ float red_min[PWM][PN], red_max[PWM][PN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % PWM, wn = wave / PWM;
    const int row0 = blockIdx.x * PM, col0 = blockIdx.y * PN;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    const Operand Xo{X, D, 1}, Ao{A, D, 1}, none{nullptr, 0, 0};
    // This block's share of the feature copy: its PM rows, the float4 columns split evenly over the tile columns.  The loads
    // are issued BEFORE the tile product (up to CPN 16-byte pieces per thread wait in registers while the MFMAs run) and
    // stored after it: as a load-store loop behind the product the copy added 95 us to the kernel, more than a pass of its own.
    constexpr int CPN = 16;
    f32x4v cpv[CPN];
    int cp_q0 = 0, cp_width = 0, cp_items = 0;
    if (cp.x) {
        const int per = (cp.c_hi - cp.c_lo + (int)gridDim.y - 1) / (int)gridDim.y;
        cp_q0 = cp.c_lo + (int)blockIdx.y * per;
        cp_width = max(0, min(cp.c_hi, cp_q0 + per) - cp_q0);
        cp_items = min(PM, N - row0) * cp_width;
        const f32x4v *src = reinterpret_cast<const f32x4v *>(cp.x) + (size_t)row0 * cp.F4;
#pragma unroll
        for (int j = 0; j < CPN; ++j) {
            const int i = tid + 256 * j;
            if (i < cp_items) {
                const int r = i / cp_width;
                cpv[j] = __builtin_nontemporal_load(src + (size_t)r * cp.F4 + cp_q0 + (i - r * cp_width));
            }
        }
    }
    mfma_accumulate<PM, PN, PWM, PWN, LAYOUT, LAYOUT>(acc, Xo, Ao, 0, D, none, none, 0, 0, row0, col0, N, K, As, Bs);
    if (cp.x) {
#pragma unroll
        for (int j = 0; j < CPN; ++j) {
            const int i = tid + 256 * j;
            if (i < cp_items) {
                const int r = i / cp_width;
                *reinterpret_cast<f32x4v *>(out + (size_t)(row0 + r) * out_cols + 4 * (cp_q0 + (i - r * cp_width))) = cpv[j];
            }
        }
        const f32x4v *src = reinterpret_cast<const f32x4v *>(cp.x) + (size_t)row0 * cp.F4;
        for (int i = tid + 256 * CPN; i < cp_items; i += 256) {       // wider shares than CPN pieces per thread (F > 1000 or K <= 128)
            const int r = i / cp_width, q = cp_q0 + (i - r * cp_width);
            *reinterpret_cast<f32x4v *>(out + (size_t)(row0 + r) * out_cols + 4 * q) = __builtin_nontemporal_load(src + (size_t)r * cp.F4 + q);
        }
    }

    // epilogue (pairwise_epilogue.h): C/D layout col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
    // It is instruction-bound (32 outputs per thread), so everything that depends on the row only is hoisted out of the
    // tile loop.  80 -> ~25 instructions per output: 48 us -> 15 us of the kernel.
    const float inf = __builtin_huge_valf();
    const int row_base = row0 + wm * 32 + 4 * (lane >> 5);
    float xr[16];                                                      // |x|^2 (euclidean) or 1 / |x| (cosine): the component the metric uses
    long long obase[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row_base + (r & 3) + 8 * (r >> 2);
        const float2 xn = row < N ? xx[row] : make_float2(1.0f, 1.0f);
        xr[r] = metric == POPE_METRIC_EUCLIDEAN ? xn.x : xn.y;
        obase[r] = (long long)row * out_cols + c0;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int cl = wn * (PN / PWN) + t * 32 + (lane & 31);            // column inside the block
        const int col = col0 + cl;
        const bool col_ok = col < K;
        const float2 an = col_ok ? aa[col] : make_float2(0.0f, 1.0f);
        float cmin = inf, cmax = -inf;
        float e[16];
        pw_metric_epilogue<false>(e, acc[t], xr, an.x, an.y, metric, row_base, N, col_ok, col, X, D, lane, [&](int acol) { return A + (size_t)acol * D; });
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (row_base + (r & 3) + 8 * (r >> 2) < N && col_ok) {
                out[obase[r] + col] = e[r];
                cmin = fminf(cmin, e[r]);
                cmax = fmaxf(cmax, e[r]);
            }
        }
        cmin = fminf(cmin, __shfl_xor(cmin, 32));
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
        if (lane < 32) {
            red_min[wm][cl] = cmin;
            red_max[wm][cl] = cmax;
        }
    }
    __syncthreads();
    if (tid < PN && col0 + tid < K) {
        float mn = red_min[0][tid], mx = red_max[0][tid];
#pragma unroll
        for (int w = 1; w < PWM; ++w) {
            mn = fminf(mn, red_min[w][tid]);
            mx = fmaxf(mx, red_max[w][tid]);
        }
        part_min[(size_t)blockIdx.x * Kpad + col0 + tid] = mn;
        part_max[(size_t)blockIdx.x * Kpad + col0 + tid] = mx;
    }
}

// Column min / max over the per-block partials, two stages (a single pass over ~1 400 partial rows by one thread per
// column is a 400 us chain of dependent loads): stage 1 folds the partial rows into RSPLIT rows, stage 2 finishes and
// applies sklearn MinMaxScaler.fit (_data.py:456-567) with feature_range (0, 1), all in float32.
constexpr int RSPLIT = 64;

__global__ __launch_bounds__(256) void k_minmax_fold(const float *__restrict__ part_min, const float *__restrict__ part_max,
                                                     int nblocks, int K, int Kpad, float *__restrict__ fold_min,
                                                     float *__restrict__ fold_max) {
    __shared__ float smin[4][64], smax[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const int per = (nblocks + RSPLIT - 1) / RSPLIT;
    const int b0 = blockIdx.y * per, b1 = min(nblocks, b0 + per);
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    if (j < K)
        for (int b = b0 + wave; b < b1; b += 4) {
            mn = fminf(mn, part_min[(size_t)b * Kpad + j]);
            mx = fmaxf(mx, part_max[(size_t)b * Kpad + j]);
        }
    smin[wave][lane] = mn;
    smax[wave][lane] = mx;
    __syncthreads();
    if (wave == 0 && j < K) {
        fold_min[(size_t)blockIdx.y * Kpad + j] = fminf(fminf(smin[0][lane], smin[1][lane]), fminf(smin[2][lane], smin[3][lane]));
        fold_max[(size_t)blockIdx.y * Kpad + j] = fmaxf(fmaxf(smax[0][lane], smax[1][lane]), fmaxf(smax[2][lane], smax[3][lane]));
    }
}

__global__ __launch_bounds__(256) void k_minmax_reduce(const float *__restrict__ fold_min, const float *__restrict__ fold_max,
                                                       int K, int Kpad, float *__restrict__ scale,
                                                       float *__restrict__ shift) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= K) return;
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
#pragma unroll 8
    for (int b = 0; b < RSPLIT; ++b) {
        mn = fminf(mn, fold_min[(size_t)b * Kpad + j]);
        mx = fmaxf(mx, fold_max[(size_t)b * Kpad + j]);
    }
    float range = mx - mn;
    if (range < 10.0f * 1.1920929e-07f) range = 1.0f;             // _handle_zeros_in_scale: < 10 * eps -> 1
    const float sc = 1.0f / range;
    scale[j] = sc;
    shift[j] = 0.0f - __fmul_rn(mn, sc);
}

// Both stages in one launch when there are few partial rows (the persistent kernel leaves one per CU): block = 64 columns,
// its sixteen waves fold rows wave, wave + 16, ..., then wave 0 finishes as k_minmax_reduce does.
__global__ __launch_bounds__(1024) void k_minmax_finish(const float *__restrict__ part_min, const float *__restrict__ part_max, int nrows,
                                                        int K, int Kpad, float *__restrict__ scale, float *__restrict__ shift) {
    __shared__ float smin[16][64], smax[16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    if (j < K) {
#pragma unroll 4
        for (int b = wave; b < nrows; b += 16) {
            mn = fminf(mn, part_min[(size_t)b * Kpad + j]);
            mx = fmaxf(mx, part_max[(size_t)b * Kpad + j]);
        }
    }
    smin[wave][lane] = mn;
    smax[wave][lane] = mx;
    __syncthreads();
    if (wave == 0 && j < K) {
#pragma unroll
        for (int w = 1; w < 16; ++w) {
            mn = fminf(mn, smin[w][lane]);
            mx = fmaxf(mx, smax[w][lane]);
        }
        float range = mx - mn;
        if (range < 10.0f * 1.1920929e-07f) range = 1.0f;
        const float sc = 1.0f / range;
        scale[j] = sc;
        shift[j] = 0.0f - __fmul_rn(mn, sc);
    }
}

// MinMaxScaler.transform: X *= scale_; X += min_  (two separately rounded operations: plain operators under contract(off);
// HIP's __fmul_rn / __fadd_rn wrappers are plain operators too and would let hipcc's default -ffp-contract=fast fuse them).
#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void k_minmax_apply(float *__restrict__ out, int N, int K, long long out_cols, int c0,
                                                      const float *__restrict__ scale, const float *__restrict__ shift) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int v = wave; v < N; v += nwaves) {
        float *row = out + (size_t)v * out_cols + c0;
        for (int j = lane; j < K; j += 64) {
            const float scaled = row[j] * scale[j];
            row[j] = scaled + shift[j];
        }
    }
}

// The same on 16-byte pieces (K, c0, out_cols multiples of 4, aligned bases): a lane owns four columns of a row, a wave one row per
// pass -- the whole 1 KB of a 256-anchor row in ONE load and ONE store instruction, where the scalar form above issues four
// load - wait - store rounds of 256 bytes (round 4: the finalise kernel's lesson).  The arithmetic per element is
// identical: two separately rounded operations.
__global__ __launch_bounds__(256) void k_minmax_apply4(float *__restrict__ out, int N, int K4, long long out_cols, int c0,
                                                       const float *__restrict__ scale, const float *__restrict__ shift) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q0 = 0; q0 < K4; q0 += 64) {                       // one trip for K <= 256
        const int q = q0 + lane;
        if (q >= K4) continue;
        const float4 sc = reinterpret_cast<const float4 *>(scale)[q], sh = reinterpret_cast<const float4 *>(shift)[q];
        for (int v = wave; v < N; v += nwaves) {
            float4 *p = reinterpret_cast<float4 *>(out + (size_t)v * out_cols + c0) + q;
            float4 e = *p;
            e.x = e.x * sc.x; e.x = e.x + sh.x;
            e.y = e.y * sc.y; e.y = e.y + sh.y;
            e.z = e.z * sc.z; e.z = e.z + sh.z;
            e.w = e.w * sc.w; e.w = e.w + sh.w;
            *p = e;
        }
    }
}

#pragma clang fp contract(fast)

// The scratch buffer of a call: every offset and the total, for both size queries and the launcher.
struct PwScratch {
    size_t xx, aa, pmin, pmax, fmin, fmax, scale, shift, rows, total;
    int part_rows, Kpad;
};

static PwScratch pw_scratch(int64_t N, int32_t K, int32_t D, bool by_id) {
    PwScratch S;
    const int64_t nblocks = (N + PM - 1) / PM;
    S.part_rows = (int)std::max<int64_t>(nblocks, 2 * std::min<int64_t>((N + PP_ROWS - 1) / PP_ROWS, PP_MAX_GRID));   // either tile kernel's partial rows fit
    S.Kpad = (K + PN - 1) / PN * PN;
    size_t o = 0;
    S.xx = o;    o += align_up((size_t)N * sizeof(float2), 256);
    S.aa = o;    o += align_up((size_t)K * sizeof(float2), 256);
    S.pmin = o;  o += align_up((size_t)S.part_rows * S.Kpad * sizeof(float), 256);
    S.pmax = o;  o += align_up((size_t)S.part_rows * S.Kpad * sizeof(float), 256);
    S.fmin = o;  o += align_up((size_t)RSPLIT * S.Kpad * sizeof(float), 256);
    S.fmax = o;  o += align_up((size_t)RSPLIT * S.Kpad * sizeof(float), 256);
    S.scale = o; o += align_up((size_t)K * sizeof(float), 256);
    S.shift = o; o += align_up((size_t)K * sizeof(float), 256);
    S.rows = o;  o += by_id ? align_up((size_t)K * D * sizeof(float), 256) : 0;   // PW_GATHER_ANCHOR_ROWS: the anchor rows as a matrix
    S.total = o;
    return S;
}

// ---- which kernels a call runs, and in which order: decided HERE and nowhere else (no HIP calls, no pointers, no globals) ----
// pairwise_plan writes the call down as an ordered list of steps with their parameters (the file header names them).
// pairwise_features_impl walks the list and launches, pope_pairwise_kernel_name walks it and prints: one switch each, without a
// default, so a step that one of them forgets is a -Wall warning.
enum PwStep : unsigned char {
    PW_CONCAT, PW_GATHER_ANCHOR_ROWS, PW_SQNORM, PW_ONE_TILE, PW_SIDE_FORK, PW_PERSISTENT, PW_SIDE_COPY, PW_MINMAX_FOLD, PW_MINMAX_REDUCE,
    PW_MINMAX_FINISH, PW_MINMAX_APPLY, PW_SIDE_JOIN
};
// 16-byte alignment of the operands; scratch: the buffer's base, and with it the scale / shift vectors and the gathered anchor rows
struct PwAligned { bool X, A, x, out, scratch; };
struct PwPlan {
    PwStep steps[8];               // in launch order (the longest call: pipeline (B) with PW_CONCAT and PW_GATHER_ANCHOR_ROWS, seven)
    int n_steps;
    void add(PwStep s) { steps[n_steps++] = s; }
    bool carries_x;                // x is still to be copied behind PW_CONCAT's place: by PW_SIDE_COPY, or inside PW_ONE_TILE
    bool vec;                      // PW_SQNORM: k_sqnorm<vec>; PW_ONE_TILE: k_pairwise<LAYOUT_KC_VEC> or <LAYOUT_GENERIC>
    unsigned sqnorm_grid;
    unsigned tile_x, tile_y;       // PW_ONE_TILE, PW_PERSISTENT: the grid; tile_x is also the number of partial rows PW_MINMAX_FOLD reads
    int copy_F4;                   // PW_ONE_TILE: the PwCopy extent, float4 columns [0, copy_F4) of x (0: no copy)
    int sets;                      // PW_PERSISTENT: consumer sets
    int finish_rows;               // PW_MINMAX_FINISH: partial rows (one per block and consumer set)
    bool apply_vec;                // PW_MINMAX_APPLY: k_minmax_apply4 (16-byte pieces) or k_minmax_apply
    unsigned apply_grid;
};

// has_x: the caller gave feature columns; side_copy_slot: the device has a side stream (SideCopy::has_slot); knob: POPE_KNOB_PAIRWISE_KERNEL.
static PwPlan pairwise_plan(int64_t N, int32_t D, int32_t K, int32_t F, int64_t out_cols, int32_t c0, bool has_x, bool by_id, const PwAligned &al,
                            bool side_copy_slot, int cus, int knob) {
    PwPlan p{};
    // the persistent kernel: depths up to 128 in 16-byte pieces, 32-bit store offsets into out
    const bool persistent = knob != 1 && D <= PP_DMAX && (D & 3) == 0 && al.X && (by_id || al.A) && (uint64_t)N * (uint64_t)out_cols * 4u < (1ull << 32);
    // The feature copy.  Both fused forms want 16-byte pieces; the side copy beside the persistent kernel also rows of at most 16 pieces
    // per lane (F <= 4096) and a slot.  What the pipeline's own form cannot take runs as a pass of its own, in front -- so pipeline (B)
    // carries a wide copy (F > 4096) that (A) hands to pope_concat.
    bool x = has_x && F > 0;
    const bool pieces = (F & 3) == 0 && (out_cols & 3) == 0 && al.x && al.out;
    if (x && !(persistent ? SideCopy::fits(F, out_cols, N, pieces) && side_copy_slot : pieces)) {
        p.add(PW_CONCAT);
        x = false;
    }
    p.carries_x = x;
    p.apply_vec = (K & 3) == 0 && (c0 & 3) == 0 && (out_cols & 3) == 0 && al.out && al.scratch;
    // apply4: one row per wave, short-lived waves in row order (the finalise kernel's grid rule)
    p.apply_grid = p.apply_vec ? (unsigned)std::min<int64_t>(std::max<int64_t>((N + 3) / 4, 256), 32768) : capped_grid((size_t)N * 64, 256);
    if (persistent) {
        // Two consumer sets keep the matrix cores busy through the epilogues; with the feature copy beside the kernel the call is
        // HBM-bound and the second set's registers are worth more to the copy's waves (configs[2]: 0.193 ms against 0.205).
        p.sets = knob == 2 ? 1 : knob == 3 ? 2 : (x ? 1 : 2);
        p.tile_x = (unsigned)std::min<int64_t>(std::min(cus, PP_MAX_GRID), (N + PP_ROWS - 1) / PP_ROWS);
        p.tile_y = (unsigned)((K + PP_COLS - 1) / PP_COLS);
        p.finish_rows = p.sets * (int)p.tile_x;
        // The copy is forked onto the side stream in front and joined at the end.  Its kernel is enqueued AFTER the tile kernel, so
        // that one's blocks (one per CU, the whole LDS) are resident first and the copy fills the wave slots they leave; started
        // first, the copy's blocks kept a quarter of the CUs busy until it ended and the tile kernel ran 139 us instead of 80.
        if (x) p.add(PW_SIDE_FORK);
        p.add(PW_PERSISTENT);
        if (x) p.add(PW_SIDE_COPY);
        p.add(PW_MINMAX_FINISH);
        p.add(PW_MINMAX_APPLY);
        if (x) p.add(PW_SIDE_JOIN);
        return p;
    }
    if (by_id) p.add(PW_GATHER_ANCHOR_ROWS);                       // the round-1 pipeline wants the anchor rows as a matrix
    p.vec = (D & 3) == 0 && al.X && (by_id ? al.scratch : al.A);   // = pick_layout(...) == LAYOUT_KC_VEC for both operands
    p.sqnorm_grid = capped_grid((size_t)(N + K) * (p.vec ? 16 : 64), 256);
    p.tile_x = (unsigned)((N + PM - 1) / PM);
    p.tile_y = (unsigned)((K + PN - 1) / PN);
    p.copy_F4 = x ? F / 4 : 0;
    p.add(PW_SQNORM);
    p.add(PW_ONE_TILE);
    p.add(PW_MINMAX_FOLD);
    p.add(PW_MINMAX_REDUCE);
    p.add(PW_MINMAX_APPLY);
    return p;
}

template <int LAYOUT, class... Args>
static int launch_one_tile(dim3 grid, hipStream_t stream, Args... args) {
    const size_t lds = tile_lds_bytes<PM, PN>();
    static LdsOptIn lds_opt_in;
    if (!lds_opt_in.done()) {
        POPE_HIP(hipFuncSetAttribute((const void *)k_pairwise<LAYOUT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_opt_in.mark();
    }
    hipLaunchKernelGGL(k_pairwise<LAYOUT>, grid, dim3(256), lds, stream, args...);
    return POPE_OK;
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace pope

using namespace pope;

// rows[j, :] = X[ids[j], :] (one wave per anchor): the anchor matrix for the kernel path that cannot follow the ids
__global__ __launch_bounds__(64) void k_gather_anchor_rows(const float *__restrict__ X, const long long *__restrict__ ids, int N, int D, float *__restrict__ rows) {
    const float *src = X + anchor_row(ids, blockIdx.x, N) * D;       // out-of-range ids are clamped (pairwise_persistent.h)
    for (int c = threadIdx.x; c < D; c += 64) rows[(size_t)blockIdx.x * D + c] = src[c];
}

extern "C" size_t pope_pairwise_scratch_bytes(int64_t N, int32_t K, int32_t D) {
    if (N <= 0 || K <= 0) return 0;
    return pw_scratch(N, K, D, false).total;
}

// anchor_ids == nullptr: A holds the K anchor rows.  Otherwise anchor j is row anchor_ids[j] of X (device int64) and A is unused:
// the persistent kernel reads the rows through the ids, the other pipeline gathers them into the scratch buffer first.
static int pairwise_features_impl(const float *x, int32_t F, const float *X, int64_t N, int32_t D, const float *A, const long long *anchor_ids, int32_t K,
                                      int32_t metric, float *out, int64_t out_cols, int32_t c0, void *scratch, size_t scratch_bytes,
                                      void *stream_) {
    clear_error();
    hipStream_t stream = (hipStream_t)stream_;
    POPE_REQUIRE(X && (A || anchor_ids) && out && scratch, "pope_pairwise_features: null pointer");
    POPE_REQUIRE(N > 0 && N < INT32_MAX && K > 0 && D > 0 && F >= 0 && c0 >= 0 && out_cols >= (int64_t)c0 + K, "pope_pairwise_features: bad size");
    POPE_REQUIRE(!x || c0 >= F, "pope_pairwise_features: the embedding columns (c0 = %d) overlap the %d feature columns", c0, F);
    POPE_REQUIRE(metric >= 0 && metric <= 2, "pope_pairwise_features: unknown metric %d", metric);
    const PwAligned al{aligned16(X), aligned16(A), aligned16(x), aligned16(out), aligned16(scratch)};
    int cus = 0, rc = device_cu_count(&cus);
    if (rc) return rc;
    const PwPlan plan = pairwise_plan(N, D, K, F, out_cols, c0, x != nullptr, anchor_ids != nullptr, al, x && SideCopy::has_slot(), cus, g_pairwise_kernel);
    const PwScratch S = pw_scratch(N, K, D, anchor_ids != nullptr);
    if (scratch_bytes < S.total) {
        set_error("pope_pairwise_features: scratch %zu < %zu bytes", scratch_bytes, S.total);
        return POPE_ERR_WORKSPACE;
    }
    char *base = (char *)scratch;
    float2 *xx = (float2 *)(base + S.xx), *aa = (float2 *)(base + S.aa);
    float *pmin = (float *)(base + S.pmin), *pmax = (float *)(base + S.pmax), *fmin = (float *)(base + S.fmin), *fmax = (float *)(base + S.fmax);
    float *scale = (float *)(base + S.scale), *shift = (float *)(base + S.shift), *rows = (float *)(base + S.rows);
    const dim3 tile_grid(plan.tile_x, plan.tile_y);
    SideCopy side;
    for (int s = 0; s < plan.n_steps && !rc; ++s) {
        switch (plan.steps[s]) {
        case PW_CONCAT: rc = pope_concat(x, N, F, out, out_cols, stream_); break;    // odd widths / unaligned bases / rows wider than the side copy takes
        case PW_GATHER_ANCHOR_ROWS:
            hipLaunchKernelGGL(k_gather_anchor_rows, dim3(K), dim3(64), 0, stream, X, anchor_ids, (int)N, D, rows);
            A = rows;
            break;
        case PW_SQNORM:
            if (plan.vec) hipLaunchKernelGGL(k_sqnorm<true>, dim3(plan.sqnorm_grid), dim3(256), 0, stream, X, (long long)N, xx, A, (long long)K, aa, D);
            else hipLaunchKernelGGL(k_sqnorm<false>, dim3(plan.sqnorm_grid), dim3(256), 0, stream, X, (long long)N, xx, A, (long long)K, aa, D);
            break;
        case PW_ONE_TILE: {
            const PwCopy copy{plan.carries_x ? x : nullptr, plan.copy_F4, 0, plan.copy_F4};
            rc = plan.vec ? launch_one_tile<LAYOUT_KC_VEC>(tile_grid, stream, X, (int)N, D, A, K, metric, (const float2 *)xx, (const float2 *)aa, out,
                                                           (long long)out_cols, c0, pmin, pmax, S.Kpad, copy)
                          : launch_one_tile<LAYOUT_GENERIC>(tile_grid, stream, X, (int)N, D, A, K, metric, (const float2 *)xx, (const float2 *)aa, out,
                                                            (long long)out_cols, c0, pmin, pmax, S.Kpad, copy);
            break;
        }
        case PW_SIDE_FORK: rc = side.fork(stream); break;
        case PW_PERSISTENT: {
            static LdsOptIn lds_opt_in;
            if (!lds_opt_in.done()) {
                POPE_HIP(hipFuncSetAttribute((const void *)k_pairwise_persistent, hipFuncAttributeMaxDynamicSharedMemorySize, PP_LDS_BYTES));
                lds_opt_in.mark();
            }
            const float *zero = nullptr;
            POPE_HIP(hipGetSymbolAddress((void **)&zero, HIP_SYMBOL(g_sk_zero)));
            const PpArgs a{X, anchor_ids ? X : A, anchor_ids, (int)N, D, K, metric, xx, out, (unsigned)out_cols, c0, pmin, pmax, S.Kpad, zero, plan.sets};
            hipLaunchKernelGGL(k_pairwise_persistent, tile_grid, dim3(PP_THREADS), PP_LDS_BYTES, stream, a);
            break;
        }
        case PW_SIDE_COPY: rc = side.launch(x, F, out, out_cols, N); break;
        case PW_MINMAX_FOLD:
            hipLaunchKernelGGL(k_minmax_fold, dim3((K + 63) / 64, RSPLIT), dim3(256), 0, stream, pmin, pmax, (int)plan.tile_x, K, S.Kpad, fmin, fmax);
            break;
        case PW_MINMAX_REDUCE: hipLaunchKernelGGL(k_minmax_reduce, dim3((K + 255) / 256), dim3(256), 0, stream, fmin, fmax, K, S.Kpad, scale, shift); break;
        case PW_MINMAX_FINISH:
            hipLaunchKernelGGL(k_minmax_finish, dim3((K + 63) / 64), dim3(1024), 0, stream, pmin, pmax, plan.finish_rows, K, S.Kpad, scale, shift);
            break;
        case PW_MINMAX_APPLY:
            if (plan.apply_vec) hipLaunchKernelGGL(k_minmax_apply4, dim3(plan.apply_grid), dim3(256), 0, stream, out, (int)N, K / 4, (long long)out_cols, c0, scale, shift);
            else hipLaunchKernelGGL(k_minmax_apply, dim3(plan.apply_grid), dim3(256), 0, stream, out, (int)N, K, (long long)out_cols, c0, scale, shift);
            break;
        case PW_SIDE_JOIN: rc = side.join(stream); break;
        }
    }
    if (rc) return rc;
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

// The plan of a call printed: c0 = F, out_cols = F + K, a device with a side-stream slot.  Bit i of `misaligned`: field i of PwAligned is
// not 16-byte aligned.
extern "C" int pope_pairwise_kernel_name_at(int64_t N, int32_t D, int32_t K, int32_t F, int32_t has_x, int32_t by_id, int32_t cu_count,
                                            uint32_t misaligned, char *name, size_t cap) {
    clear_error();
    POPE_REQUIRE(name && cap > 0 && N > 0 && N < INT32_MAX && D > 0 && K > 0 && F >= 0 && cu_count > 0 && misaligned < (1u << 5),
                 "pope_pairwise_kernel_name: bad argument");
    const auto ok = [misaligned](int bit) { return !(misaligned >> bit & 1u); };
    const PwPlan p = pairwise_plan(N, D, K, F, (int64_t)F + K, F, has_x != 0, by_id != 0, PwAligned{ok(0), ok(1), ok(2), ok(3), ok(4)}, true, cu_count,
                                   g_pairwise_kernel);
    char buf[256];
    int n = 0;
    auto add = [&](const char *fmt, auto... args) {
        if (n < (int)sizeof buf) n += snprintf(buf + n, sizeof buf - n, "%s", n ? "+" : "");
        if (n < (int)sizeof buf) n += snprintf(buf + n, sizeof buf - n, fmt, args...);
    };
    for (int s = 0; s < p.n_steps; ++s) {
        switch (p.steps[s]) {
        case PW_CONCAT:             add("%s", "pope_concat"); break;
        case PW_GATHER_ANCHOR_ROWS: add("%s", "k_gather_anchor_rows"); break;
        case PW_SQNORM:             add("k_sqnorm<%s>", p.vec ? "true" : "false"); break;
        case PW_ONE_TILE:           add("k_pairwise<%d>%s", p.vec ? (int)LAYOUT_KC_VEC : (int)LAYOUT_GENERIC, p.copy_F4 ? "[copy]" : ""); break;
        case PW_SIDE_FORK:          break;                           // (stream events: no kernel)
        case PW_PERSISTENT:         add("k_pairwise_persistent[sets=%d]", p.sets); break;
        case PW_SIDE_COPY:          add("%s", "k_copy_features"); break;
        case PW_MINMAX_FOLD:        add("%s", "k_minmax_fold"); break;
        case PW_MINMAX_REDUCE:      add("%s", "k_minmax_reduce"); break;
        case PW_MINMAX_FINISH:      add("%s", "k_minmax_finish"); break;
        case PW_MINMAX_APPLY:       add("%s", p.apply_vec ? "k_minmax_apply4" : "k_minmax_apply"); break;
        case PW_SIDE_JOIN:          break;
        }
    }
    POPE_REQUIRE((size_t)n < cap && n < (int)sizeof buf, "pope_pairwise_kernel_name: %d characters do not fit name[%zu]", n, cap);
    memcpy(name, buf, (size_t)n + 1);
    return POPE_OK;
}

extern "C" int pope_pairwise_kernel_name(int64_t N, int32_t D, int32_t K, int32_t F, int32_t has_x, int32_t by_id, int32_t cu_count, char *name, size_t cap) {
    return pope_pairwise_kernel_name_at(N, D, K, F, has_x, by_id, cu_count, 0, name, cap);
}

extern "C" int pope_pairwise_features(const float *x, int32_t F, const float *X, int64_t N, int32_t D, const float *A, int32_t K,
                                      int32_t metric, float *out, int64_t out_cols, int32_t c0, void *scratch, size_t scratch_bytes,
                                      void *stream_) {
    return pairwise_features_impl(x, F, X, N, D, A, nullptr, K, metric, out, out_cols, c0, scratch, scratch_bytes, stream_);
}

// utils.py:165-167 as it is written there -- embedding[anchor_nodes] and the distances in one call: anchor j is row
// anchor_ids[j] (device int64, each in [0, N)) of X; no gathered copy of the anchor rows is made on the common path.
extern "C" size_t pope_pairwise_by_id_scratch_bytes(int64_t N, int32_t K, int32_t D) {
    if (N <= 0 || K <= 0 || D <= 0) return 0;
    return pw_scratch(N, K, D, true).total;
}

extern "C" int pope_pairwise_features_by_id(const float *x, int32_t F, const float *X, int64_t N, int32_t D, const int64_t *anchor_ids, int32_t K,
                                            int32_t metric, float *out, int64_t out_cols, int32_t c0, void *scratch, size_t scratch_bytes,
                                            void *stream_) {
    clear_error();
    POPE_REQUIRE(anchor_ids, "pope_pairwise_features_by_id: null pointer");
    return pairwise_features_impl(x, F, X, N, D, nullptr, (const long long *)anchor_ids, K, metric, out, out_cols, c0, scratch, scratch_bytes, stream_);
}

extern "C" int pope_pairwise_minmax(const float *X, int64_t N, int32_t D, const float *A, int32_t K, int32_t metric,
                                    float *out, int64_t out_cols, int32_t c0, void *scratch, size_t scratch_bytes,
                                    void *stream_) {
    return pope_pairwise_features(nullptr, 0, X, N, D, A, K, metric, out, out_cols, c0, scratch, scratch_bytes, stream_);
}

#ifdef POPE_STAMP
extern "C" int pope_debug_read_pairwise_stamps(unsigned long long *host, int count) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_pp_stamps), (size_t)count * sizeof(unsigned long long));
}
#endif
