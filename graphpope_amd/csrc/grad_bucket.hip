// Gradient bucket of data-parallel SAGE training (main.py:285-290: Trainer(gpus=n, accelerator='ddp')): the gradients of a step, which
// the autograd nodes hand out as separate tensors at fresh addresses, are packed -- pre-scaled by 1 / world -- into ONE flat float32
// buffer, so that the ranks exchange them with one all-reduce and the norm pass and the Adam step read them from addresses that stay.
//
//   layout   tensor t starts at offsets[t] = sum over s < t of round_up(numel[s], 4) float elements: every start is 16-byte aligned when
//            the buffer is, tensors in list order, up to three padding elements behind each
//   pack     flat[offsets[t] + j] = grads[t][j] * scale, the padding +0.0f; one launch per BUCKET_MAX_TENSORS tensors, in the style of
//            k_copy_segments / k_adam: descriptors and a prefix sum of blocks per tensor in the argument block.  One rounding per element,
//            no atomics, no scratch, no host synchronisation: capturable.
#include "common.h"

using namespace pope;

namespace pope {

constexpr int BUCKET_MAX_TENSORS = 32;         // descriptors per launch (0.9 KB of kernel arguments)
constexpr int BUCKET_CHUNK = 4096;             // elements per block: 16 KB in, 16 KB out, four 16-byte packs per thread

struct BucketTable {
    const float *src[BUCKET_MAX_TENSORS];
    long long n[BUCKET_MAX_TENSORS];
    long long off[BUCKET_MAX_TENSORS];         // start in `flat`, a multiple of 4 elements
    int first_block[BUCKET_MAX_TENSORS + 1];   // prefix sum of ceil(n / BUCKET_CHUNK)
    int count;
};

inline long long bucket_padded(long long n) { return (n + 3) & ~3ll; }

// A thread owns whole packs of 4 destination elements (the destination is 16-byte aligned by the layout): one 16-byte load where the
// source is aligned and the pack lies inside the tensor, scalar loads otherwise; the pack that holds the tensor's end carries the
// padding zeros.  A 2 MB model is 128 blocks: the launch, not the bandwidth, is what this costs.
__global__ __launch_bounds__(256) void k_grad_bucket_pack(BucketTable t, float scale, float *__restrict__ flat) {
    int k = 0;
    while (k + 1 < t.count && (int)blockIdx.x >= t.first_block[k + 1]) ++k;
    const long long n = t.n[k];
    const long long base = (long long)((int)blockIdx.x - t.first_block[k]) * BUCKET_CHUNK;
    const long long end = min((n + 3) & ~3ll, base + BUCKET_CHUNK);       // padded: the last pack of the tensor is written whole
    const float *__restrict__ s = t.src[k];
    float *__restrict__ d = flat + t.off[k];
    const bool aligned = (reinterpret_cast<uintptr_t>(s) & 15) == 0;
    for (long long q = base + 4ll * threadIdx.x; q < end; q += 4ll * blockDim.x) {
        float4 g;
        if (aligned && q + 4 <= n) {
            g = *reinterpret_cast<const float4 *>(s + q);
        } else {
            g.x = q < n ? s[q] : 0.f;
            g.y = q + 1 < n ? s[q + 1] : 0.f;
            g.z = q + 2 < n ? s[q + 2] : 0.f;
            g.w = q + 3 < n ? s[q + 3] : 0.f;
        }
        float4 o;
        o.x = q < n ? g.x * scale : 0.f;                                  // the padding is +0.0f whatever the scale's sign
        o.y = q + 1 < n ? g.y * scale : 0.f;
        o.z = q + 2 < n ? g.z * scale : 0.f;
        o.w = q + 3 < n ? g.w * scale : 0.f;
        *reinterpret_cast<float4 *>(d + q) = o;
    }
}

}  // namespace pope

extern "C" int64_t sage_grad_bucket_layout(int32_t n, const int64_t *numel, int64_t *offsets) {
    if (n < 0 || (n > 0 && !numel)) return -1;
    int64_t total = 0;
    for (int t = 0; t < n; ++t) {
        if (numel[t] < 0 || numel[t] > INT64_MAX - 3 - total) return -1;
        total += bucket_padded(numel[t]);
    }
    if (offsets) {
        int64_t at = 0;
        for (int t = 0; t < n; ++t) {
            offsets[t] = at;
            at += bucket_padded(numel[t]);
        }
    }
    return total;
}

extern "C" int32_t sage_grad_bucket_chunk(void) { return BUCKET_CHUNK; }
extern "C" int32_t sage_grad_bucket_table(void) { return BUCKET_MAX_TENSORS; }

extern "C" int sage_grad_bucket_pack(int32_t n, const float *const *grads, const int64_t *numel, float scale, float *flat, int64_t flat_len,
                                     void *stream_) {
    clear_error();
    POPE_REQUIRE(n >= 0 && (n == 0 || (grads && numel)), "sage_grad_bucket_pack: null pointer");
    const int64_t total = sage_grad_bucket_layout(n, numel, nullptr);
    POPE_REQUIRE(total >= 0, "sage_grad_bucket_pack: negative size in the list");
    POPE_REQUIRE(flat, "sage_grad_bucket_pack: flat is a null pointer");
    POPE_REQUIRE((reinterpret_cast<uintptr_t>(flat) & 15) == 0, "sage_grad_bucket_pack: flat must be 16-byte aligned");
    POPE_REQUIRE(flat_len >= total, "sage_grad_bucket_pack: flat holds %lld elements, the layout needs %lld", (long long)flat_len, (long long)total);
    POPE_REQUIRE(total / BUCKET_CHUNK + n < INT32_MAX, "sage_grad_bucket_pack: %lld elements are more blocks than one grid holds", (long long)total);
    for (int t = 0; t < n; ++t)                                          // the whole list first: on error nothing is launched
        POPE_REQUIRE(numel[t] == 0 || grads[t], "sage_grad_bucket_pack: tensor %d has a null pointer", t);
    int64_t at = 0;
    int t = 0;
    while (t < n) {
        BucketTable tab;
        tab.count = 0;
        int blocks = 0;
        for (; t < n && tab.count < BUCKET_MAX_TENSORS; ++t) {
            if (numel[t] == 0) continue;                                 // no elements and no padding: nothing to write
            const int c = tab.count++;
            tab.src[c] = grads[t]; tab.n[c] = numel[t]; tab.off[c] = at;
            tab.first_block[c] = blocks;
            blocks += (int)((numel[t] + BUCKET_CHUNK - 1) / BUCKET_CHUNK);
            at += bucket_padded(numel[t]);
        }
        if (tab.count == 0) continue;
        tab.first_block[tab.count] = blocks;
        hipLaunchKernelGGL(k_grad_bucket_pack, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, tab, scale, flat);
    }
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}
