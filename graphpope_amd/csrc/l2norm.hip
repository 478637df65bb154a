// L2 normalisation of the rows of a SAGEConv output, forward and backward
// (PyG 1.7.0 SAGEConv(normalize=True): out = F.normalize(out, p=2., dim=-1), eps = 1e-12; line 7 of Algorithm 1 of the GraphSAGE paper).
//
// The matrix is [M, C] float32 row-major (M = destination nodes of the hop, C = the layer's width).  Each direction is ONE launch and a
// pure stream: a wave owns a row, reads it once, folds one number over the wave and writes the row.
//   forward    ss = sum_c x[i, c]^2,  inv_norm[i] = 1 / max(sqrt(ss), eps),  y[i, :] = x[i, :] * inv_norm[i]
//   backward   d = sum_c y[i, c] * g[i, c];  grad_x[i, :] = inv_norm[i] * (g[i, :] - y[i, :] * d)      where the norm exceeded eps,
//                                            grad_x[i, :] = g[i, :] / eps                              where it was clamped
// Who sums what: columns are taken in packs of four, pack q = c / 4 belongs to lane q % 64.  A lane adds its packs in ascending order, the
// four columns of a pack in ascending order, each term by one fused multiply-add onto a float32 partial that starts at +0; the 64 partials
// are folded by wave_sum (csrc/wave.h).  The vector instantiation reads a pack as one 16-byte access, the scalar one as up to four 4-byte
// accesses -- the SAME ownership and order, so the two give the same bits and the result does not depend on where the caller's buffers
// lie.  No atomics, no scratch, no second copy of a reduction.
// A lane keeps its first L2_CACHED packs in registers between the sum and the write (C <= 1024: the row is read once); wider rows are read
// again, by the lane that read them first.  A lane writes only elements it has itself read, after the fold, and no wave touches another
// wave's row: y may be x, grad_x may be grad_y.
#include "common.h"
#include "wave.h"

namespace pope {

constexpr int L2_CACHED = 4;

// Pack q of a row of C floats; columns at or beyond C read as +0 (the scalar form only: the vector form needs C % 4 == 0).
template <bool VEC>
__device__ __forceinline__ float4 l2_load(const float *row, int q, int C) {
    if constexpr (VEC) {
        return reinterpret_cast<const float4 *>(row)[q];
    } else {
        const int c = q * 4;
        float4 v;
        v.x = row[c];                                   // q < ceil(C / 4): the first column exists
        v.y = c + 1 < C ? row[c + 1] : 0.f;
        v.z = c + 2 < C ? row[c + 2] : 0.f;
        v.w = c + 3 < C ? row[c + 3] : 0.f;
        return v;
    }
}

template <bool VEC>
__device__ __forceinline__ void l2_store(float *row, int q, int C, const float4 v) {
    if constexpr (VEC) {
        reinterpret_cast<float4 *>(row)[q] = v;
    } else {
        const int c = q * 4;
        row[c] = v.x;
        if (c + 1 < C) row[c + 1] = v.y;
        if (c + 2 < C) row[c + 2] = v.z;
        if (c + 3 < C) row[c + 3] = v.w;
    }
}

__device__ __forceinline__ float l2_dot(float s, const float4 a, const float4 b) {
    s = fmaf(a.x, b.x, s);
    s = fmaf(a.y, b.y, s);
    s = fmaf(a.z, b.z, s);
    return fmaf(a.w, b.w, s);
}

// x and y carry no __restrict__: they may be the same matrix.
template <bool VEC>
__global__ __launch_bounds__(256) void k_l2_normalize(const float *x, int M, int C, float eps, float *y, float *__restrict__ inv_norm,
                                                      const int *__restrict__ m_dev) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    const int packs = (C + 3) >> 2;
    M = dyn_extent(m_dev, M);
    for (int i = wave; i < M; i += nwaves) {
        const float *xr = x + (size_t)i * C;
        float *yr = y + (size_t)i * C;
        float4 keep[L2_CACHED];
#pragma unroll
        for (int k = 0; k < L2_CACHED; ++k) {                          // the loads first: up to four 16-byte reads in flight per lane
            const int q = lane + 64 * k;
            keep[k] = q < packs ? l2_load<VEC>(xr, q, C) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float ss = 0.f;
#pragma unroll
        for (int k = 0; k < L2_CACHED; ++k)
            if (lane + 64 * k < packs) ss = l2_dot(ss, keep[k], keep[k]);
        for (int q = lane + 64 * L2_CACHED; q < packs; q += 64) {
            const float4 v = l2_load<VEC>(xr, q, C);
            ss = l2_dot(ss, v, v);
        }
        ss = wave_sum(ss);
        const float norm = sqrtf(ss);
        const float inv = 1.0f / (norm < eps ? eps : norm);             // not fmaxf: a NaN norm must stay NaN (torch's clamp_min keeps it)
        if (lane == 0) inv_norm[i] = inv;
#pragma unroll
        for (int k = 0; k < L2_CACHED; ++k) {
            const int q = lane + 64 * k;
            if (q < packs) l2_store<VEC>(yr, q, C, make_float4(keep[k].x * inv, keep[k].y * inv, keep[k].z * inv, keep[k].w * inv));
        }
        for (int q = lane + 64 * L2_CACHED; q < packs; q += 64) {
            const float4 v = l2_load<VEC>(xr, q, C);
            l2_store<VEC>(yr, q, C, make_float4(v.x * inv, v.y * inv, v.z * inv, v.w * inv));
        }
    }
}

// Which branch a row took is read off inv_norm: the forward pass clamps with `norm < eps ? eps : norm`, so a clamped row holds exactly
// 1.0f / eps, formed here by the same correctly rounded division.  A row whose norm was at or a rounding above eps holds that value too
// and is treated as clamped; its norm is within one float32 rounding of the threshold, less than the rounding of the norm itself.
// A NaN inv_norm compares unequal and takes the projected form, which makes the whole row NaN.  g and gx may be the same matrix.
template <bool VEC>
__global__ __launch_bounds__(256) void k_l2_normalize_backward(const float *__restrict__ y, const float *__restrict__ inv_norm, const float *g,
                                                               int M, int C, float eps, float *gx, const int *__restrict__ m_dev) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    const int packs = (C + 3) >> 2;
    const float inv_eps = 1.0f / eps;
    M = dyn_extent(m_dev, M);
    for (int i = wave; i < M; i += nwaves) {
        const float *yr = y + (size_t)i * C;
        const float *gr = g + (size_t)i * C;
        float *out = gx + (size_t)i * C;
        const float inv = inv_norm[i];
        if (inv == inv_eps) {                                           // wave-uniform: the whole wave reads the same word
            for (int q = lane; q < packs; q += 64) {
                const float4 v = l2_load<VEC>(gr, q, C);
                l2_store<VEC>(out, q, C, make_float4(v.x / eps, v.y / eps, v.z / eps, v.w / eps));
            }
            continue;
        }
        float4 ky[L2_CACHED], kg[L2_CACHED];
#pragma unroll
        for (int k = 0; k < L2_CACHED; ++k) {
            const int q = lane + 64 * k;
            const bool in = q < packs;
            ky[k] = in ? l2_load<VEC>(yr, q, C) : make_float4(0.f, 0.f, 0.f, 0.f);
            kg[k] = in ? l2_load<VEC>(gr, q, C) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < L2_CACHED; ++k)
            if (lane + 64 * k < packs) d = l2_dot(d, ky[k], kg[k]);
        for (int q = lane + 64 * L2_CACHED; q < packs; q += 64) d = l2_dot(d, l2_load<VEC>(yr, q, C), l2_load<VEC>(gr, q, C));
        d = wave_sum(d);
        // each operation rounded on its own (no contraction): the product y * d, the difference, the scaling
        const auto term = [inv, d](float yv, float gv) { return __fmul_rn(inv, __fsub_rn(gv, __fmul_rn(yv, d))); };
#pragma unroll
        for (int k = 0; k < L2_CACHED; ++k) {
            const int q = lane + 64 * k;
            if (q < packs)
                l2_store<VEC>(out, q, C, make_float4(term(ky[k].x, kg[k].x), term(ky[k].y, kg[k].y), term(ky[k].z, kg[k].z), term(ky[k].w, kg[k].w)));
        }
        for (int q = lane + 64 * L2_CACHED; q < packs; q += 64) {
            const float4 a = l2_load<VEC>(yr, q, C), b = l2_load<VEC>(gr, q, C);
            l2_store<VEC>(out, q, C, make_float4(term(a.x, b.x), term(a.y, b.y), term(a.z, b.z), term(a.w, b.w)));
        }
    }
}

static bool l2_aligned(const void *a, const void *b, const void *c) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0; }

// One wave per row, four rows per block; beyond 4 096 blocks the waves stride over the rows.
static unsigned l2_grid(int64_t M) { return capped_grid((size_t)M * 64, 256); }

}  // namespace pope

using namespace pope;

extern "C" int sage_l2_normalize_forward(const float *x, int64_t M, int32_t C, float eps, float *y, float *inv_norm, const int32_t *rows_dev,
                                         void *stream_) {
    clear_error();
    POPE_REQUIRE(x && y && inv_norm, "sage_l2_normalize_forward: null pointer");
    POPE_REQUIRE(M >= 0 && M < INT32_MAX && C > 0 && (size_t)M * C < ((size_t)1 << 40), "sage_l2_normalize_forward: bad size");
    POPE_REQUIRE(eps > 0.f, "sage_l2_normalize_forward: need eps > 0");
    if (M == 0) return POPE_OK;
    hipStream_t stream = (hipStream_t)stream_;
    if (C % 4 == 0 && l2_aligned(x, y, nullptr))
        hipLaunchKernelGGL(k_l2_normalize<true>, dim3(l2_grid(M)), dim3(256), 0, stream, x, (int)M, C, eps, y, inv_norm, rows_dev);
    else
        hipLaunchKernelGGL(k_l2_normalize<false>, dim3(l2_grid(M)), dim3(256), 0, stream, x, (int)M, C, eps, y, inv_norm, rows_dev);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" int sage_l2_normalize_backward(const float *y, const float *inv_norm, const float *grad_y, int64_t M, int32_t C, float eps,
                                          float *grad_x, const int32_t *rows_dev, void *stream_) {
    clear_error();
    POPE_REQUIRE(y && inv_norm && grad_y && grad_x, "sage_l2_normalize_backward: null pointer");
    POPE_REQUIRE(M >= 0 && M < INT32_MAX && C > 0 && (size_t)M * C < ((size_t)1 << 40), "sage_l2_normalize_backward: bad size");
    POPE_REQUIRE(eps > 0.f, "sage_l2_normalize_backward: need eps > 0");
    if (M == 0) return POPE_OK;
    hipStream_t stream = (hipStream_t)stream_;
    if (C % 4 == 0 && l2_aligned(y, grad_y, grad_x))
        hipLaunchKernelGGL(k_l2_normalize_backward<true>, dim3(l2_grid(M)), dim3(256), 0, stream, y, inv_norm, grad_y, (int)M, C, eps, grad_x,
                           rows_dev);
    else
        hipLaunchKernelGGL(k_l2_normalize_backward<false>, dim3(l2_grid(M)), dim3(256), 0, stream, y, inv_norm, grad_y, (int)M, C, eps, grad_x,
                           rows_dev);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" int sage_l2_normalize_kernel_name_at(int64_t M, int32_t C, uint32_t misaligned, char *name, size_t cap) {
    clear_error();
    POPE_REQUIRE(name && cap > 0 && M > 0 && M < INT32_MAX && C > 0 && misaligned < (1u << 4), "sage_l2_normalize_kernel_name: bad argument");
    const auto ok = [misaligned](int bit) { return !(misaligned >> bit & 1u); };
    const bool fwd = C % 4 == 0 && ok(0) && ok(1), bwd = C % 4 == 0 && ok(1) && ok(2) && ok(3);
    snprintf(name, cap, "k_l2_normalize<%s>+k_l2_normalize_backward<%s>", fwd ? "true" : "false", bwd ? "true" : "false");
    return POPE_OK;
}
