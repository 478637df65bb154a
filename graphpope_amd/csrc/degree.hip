// Biased anchor selection on the device: sampling_method='degree_centrality', the command line's default.
//
// Replaces /root/reference/utils.py:38-42  nx.degree_centrality(to_networkx(data)), the ascending stable sort of its scores
// and the slice that keeps the last K.  Two parts:
//
// 1. Degrees.  On the DiGraph the degree of v is its in-degree plus its out-degree over DISTINCT (u, v) pairs; a self-loop
//    counts 2.  In the canonical CSR by source (pope_csr_build_canonical: every row's targets ascending) repeated edges are
//    adjacent, so slot p is the first of its pair iff  p == rowptr[erow[p]] || col[p] != col[p - 1],  and only such slots add
//    1 to deg[erow[p]] (summed over the run of a row inside a wave first) and 1 to deg[col[p]].  32-bit integer atomics (deg <= 2 N < 2^32): exact, the same on every run.  The
//    counters ARE the low words of the int64 result (little endian, high words zeroed first), so nothing is widened afterwards.
//    nx.degree_centrality multiplies by 1 / (n - 1): strictly monotone in the integer, so ranking by the integer is ranking
//    by NetworkX's float.  key[v] = deg[v] << 32 | v makes all keys distinct: "ascending stable sort by score, keep the last
//    K" is exactly "the K largest keys, ascending", the node ids in the low words.
//
// 2. pope_topk_u64: the K largest of N unsigned 64-bit keys (any keys, duplicates allowed), ascending -- a radix select, not
//    a sort of N.  Nine launches walk the eight digits from the most significant one; launch D
//      - narrows: from the histogram of digit D - 1 (over the keys that share the prefix so far) it finds the bin that holds the
//        K-th largest key, appends it to the prefix and subtracts the keys in the bins above from "how many still to take"
//        (every block derives the same answer from the same 256 counts; block 0 records it),
//      - filters the candidates of launch D - 1 by that digit: above the bin -> straight into the result (they are among the K
//        largest), in the bin -> the next candidate buffer and the histogram of digit D, below -> dropped.  If the digit
//        narrowed nothing (every candidate in the bin) nothing is copied and the next launch reads the same candidates again.
//    After digit 7 the prefix is the K-th largest key T itself and `remaining` the number of copies of T still to take: they
//    fill the result's tail.  A one-block bitonic sort in LDS orders the K keys.  Histograms: LDS atomics per block, then one
//    global add per non-empty bin per block; compaction: a ballot and one atomic per wave.  The state lives in the scratch and
//    never visits the host; the call clears every counter it reads.
#include "common.h"

namespace pope {

constexpr int TOPK_BLOCK = 256;       // one thread per bin in the narrowing step
constexpr int TOPK_SORT_THREADS = 1024;
constexpr unsigned TOPK_GRID_CAP = 1024;

// ---------------------------------------------------------------------------------------------------------- degrees
__global__ __launch_bounds__(256) void k_degree_count(const int *__restrict__ rowptr, const int *__restrict__ col,
                                                      const int *__restrict__ erow, int N, unsigned *__restrict__ deg_lo) {
    const size_t E = (size_t)rowptr[N];                           // the slots; col / erow are padded beyond with anything
    const int lane = threadIdx.x & 63;
    for (size_t base = (size_t)blockIdx.x * blockDim.x; base < E; base += (size_t)gridDim.x * blockDim.x) {   // whole waves enter
        const size_t p = base + threadIdx.x;
        const bool valid = p < E;
        int r = -1, c = 0;
        bool first = false;                                       // first slot of its (r, c) pair
        if (valid) {
            r = erow[p];
            c = col[p];
            first = p == (size_t)rowptr[r] || col[p - 1] != c;
        }
        if (first) atomicAdd(&deg_lo[2 * (size_t)c], 1u);         // in-degree: one add per distinct pair
        // out-degree: the slots are sorted by row, so equal rows are runs of neighbouring lanes; the first lane of a run adds
        // the run's distinct pairs in one atomic (per-slot adds: 8.3 ms against 3.2 ms on R-MAT-22)
        const int r_prev = __shfl_up(r, 1, 64);
        const unsigned long long heads = __ballot(valid && (lane == 0 || r != r_prev));
        const unsigned long long firsts = __ballot(first);
        if (valid && ((heads >> lane) & 1ull)) {
            const unsigned long long later = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
            const unsigned long long below_next = later ? (1ull << (__ffsll((long long)later) - 1)) - 1ull : ~0ull;
            const unsigned cnt = (unsigned)__popcll(firsts & below_next & (~0ull << lane));
            if (cnt) atomicAdd(&deg_lo[2 * (size_t)r], cnt);
        }
    }
}

__global__ __launch_bounds__(256) void k_degree_keys(const long long *__restrict__ deg, int N, u64 *__restrict__ keys) {
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < N; v += gridDim.x * blockDim.x)
        keys[v] = ((u64)deg[v] << 32) | (u64)(unsigned)v;
}

// ---------------------------------------------------------------------------------------------------------- top-K select
struct TopkState {                    // after D digits:
    u64 prefix;                       // the top D digits of the K-th largest key (lower digits zero)
    unsigned remaining;               // how many keys with that prefix are still to take (>= 1)
    unsigned n;                       // how many keys have that prefix = the candidates the next launch reads ...
    unsigned src;                     // ... from here: 0 = the caller's keys, 1 / 2 = a candidate buffer
    unsigned pad;
};

struct TopkCtl {
    TopkState st[9];                  // st[D] for D = 1 .. 8 (st[0] = {0, K, N, 0} comes from the arguments)
    unsigned cursor[9];               // candidates written by launch D
    unsigned emitted;                 // keys written to the result so far
};

struct TopkScratch {
    size_t ctl, hist, cand, total;
};

__host__ __device__ inline TopkScratch topk_layout(size_t N) {
    TopkScratch L;
    size_t o = 0;
    L.ctl = o;  o += (sizeof(TopkCtl) + 255) / 256 * 256;
    L.hist = o; o += 8 * 256 * sizeof(unsigned);
    L.cand = o; o += (2 * N * sizeof(u64) + 255) / 256 * 256;     // two candidate buffers, read one / write the other
    L.total = o;
    return L;
}

// pos of this lane among the lanes of `mask`, after one atomic of the wave on *counter (mask != 0, wave-uniform).
__device__ __forceinline__ unsigned wave_slot(unsigned long long mask, unsigned *counter, int lane) {
    const int leader = __ffsll((long long)mask) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(mask));
    base = (unsigned)__shfl((int)base, leader, 64);
    return base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
}

template <int D>
__global__ __launch_bounds__(TOPK_BLOCK) void k_topk_pass(const u64 *__restrict__ keys, unsigned N, unsigned K, TopkCtl *__restrict__ ctl,
                                                          unsigned *__restrict__ hist, u64 *__restrict__ cand, u64 *__restrict__ out) {
    __shared__ unsigned h[256];
    __shared__ unsigned sel[2];
    const int t = threadIdx.x, lane = t & 63;
    constexpr int PREV_SHIFT = D >= 1 ? 64 - 8 * D : 0;           // digit D - 1
    constexpr int SHIFT = D <= 7 ? 56 - 8 * D : 0;                // digit D
    TopkState prev = {0ull, K, N, 0u, 0u}, cur = prev;
    unsigned bin = 0;
    bool copy = false;                                            // this launch writes a candidate buffer
    if constexpr (D >= 1) {
        if constexpr (D >= 2) prev = ctl->st[D - 1];
        const unsigned c = hist[(D - 1) * 256 + t];
        h[t] = c;
        if (t == 0) sel[0] = sel[1] = 0;
        __syncthreads();
        unsigned above = 0;                                       // keys in the bins above mine
        for (int j = t + 1; j < 256; ++j) above += h[j];
        if (above < prev.remaining && prev.remaining <= above + c) {   // exactly one bin: 1 <= remaining <= sum of the bins
            sel[0] = (unsigned)t;
            sel[1] = above;
        }
        __syncthreads();
        bin = sel[0];
        cur.prefix = prev.prefix | ((u64)bin << PREV_SHIFT);
        cur.remaining = prev.remaining - sel[1];
        cur.n = h[bin];
        cur.src = prev.src;
        if constexpr (D <= 7) {
            // a digit that narrows nothing (the high digits of small keys, runs of equal keys) keeps the candidates where they
            // are: the next launch reads the same buffer again and no wave queues at the cursor
            copy = cur.n != prev.n;
            if (copy) cur.src = prev.src == 1u ? 2u : 1u;
        }
        if (blockIdx.x == 0 && t == 0) ctl->st[D] = cur;
        __syncthreads();
    }
    h[t] = 0;
    __syncthreads();
    const u64 *src = prev.src == 0u ? keys : cand + (size_t)(prev.src - 1u) * N;
    u64 *dst = cand + (size_t)(cur.src == 2u ? 1u : 0u) * N;      // written only if `copy`
    const size_t n = prev.n < N ? prev.n : N;                     // D <= 1: N
    for (size_t base = (size_t)blockIdx.x * TOPK_BLOCK; base < n; base += (size_t)gridDim.x * TOPK_BLOCK) {   // whole waves enter
        const size_t i = base + t;
        const bool valid = i < n;
        const u64 key = valid ? src[i] : 0ull;
        bool keep = valid;
        if constexpr (D >= 1) {
            const unsigned dp = (unsigned)(key >> PREV_SHIFT) & 255u;
            const bool emit = valid && dp > bin;
            keep = valid && dp == bin;
            const unsigned long long em = __ballot(emit);
            if (em) {
                const unsigned pos = wave_slot(em, &ctl->emitted, lane);
                if (emit && pos < K) out[pos] = key;
            }
        }
        if constexpr (D <= 7) {
            const unsigned long long km = __ballot(keep);
            if (km) {
                if (copy) {
                    const unsigned pos = wave_slot(km, &ctl->cursor[D], lane);
                    if (keep && pos < N) dst[pos] = key;
                }
                const unsigned dg = (unsigned)(key >> SHIFT) & 255u;
                const unsigned d0 = (unsigned)__shfl((int)dg, __ffsll((long long)km) - 1, 64);
                if (__ballot(keep && dg == d0) == km) {           // the whole wave in one bin (the high digits of small keys)
                    if (lane == __ffsll((long long)km) - 1) atomicAdd(&h[d0], (unsigned)__popcll(km));
                } else if (keep) {
                    atomicAdd(&h[dg], 1u);
                }
            }
        }
    }
    if constexpr (D <= 7) {
        __syncthreads();
        const unsigned c = h[t];
        if (c) atomicAdd(&hist[D * 256 + t], c);
    }
    if (D == 8 && blockIdx.x == 0)                                // the copies of T itself: the result's tail
        for (unsigned i = t; i < cur.remaining; i += TOPK_BLOCK) out[K - cur.remaining + i] = cur.prefix;
}

// Bitonic sort of out[0, K) in LDS, padded to P = the power of two >= K with the largest key (the pads sort to the end).
__global__ __launch_bounds__(TOPK_SORT_THREADS) void k_topk_sort(u64 *__restrict__ out, int K, int P) {
    __shared__ u64 s[POPE_TOPK_MAX_K];
    const int t = threadIdx.x;
    for (int i = t; i < P; i += TOPK_SORT_THREADS) s[i] = i < K ? out[i] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += TOPK_SORT_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const u64 a = s[i], b = s[x];
                    if ((a > b) == ((i & k) == 0)) {
                        s[i] = b;
                        s[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = t; i < K; i += TOPK_SORT_THREADS) out[i] = s[i];
}

}  // namespace pope

using namespace pope;

static_assert((POPE_TOPK_MAX_K & (POPE_TOPK_MAX_K - 1)) == 0 && POPE_TOPK_MAX_K >= 1024 && POPE_TOPK_MAX_K * sizeof(u64) <= 64 * 1024,
              "POPE_TOPK_MAX_K: a power of two that the one-block LDS sort holds");

namespace {

bool topk_sizes_ok(int64_t N, int64_t K) { return N > 0 && N < INT32_MAX && K >= 1 && K <= N && K <= POPE_TOPK_MAX_K; }

template <int D>
void topk_launch(unsigned grid, hipStream_t stream, const u64 *keys, unsigned N, unsigned K, TopkCtl *ctl, unsigned *hist, u64 *cand,
                 u64 *out) {
    hipLaunchKernelGGL(k_topk_pass<D>, dim3(grid), dim3(TOPK_BLOCK), 0, stream, keys, N, K, ctl, hist, cand, out);
}

}  // namespace

extern "C" int pope_degree_counts(const int32_t *rowptr, const int32_t *col, const int32_t *erow, int64_t N, int64_t *degree,
                                  uint64_t *keys, void *stream_) {
    clear_error();
    POPE_REQUIRE(N > 0 && N < INT32_MAX, "pope_degree_counts: need 0 < N < 2^31 (N=%lld)", (long long)N);
    POPE_REQUIRE(rowptr && col && erow && degree, "pope_degree_counts: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    POPE_HIP(hipMemsetAsync(degree, 0, (size_t)N * sizeof(int64_t), stream));
    // E = rowptr[N] is on the device: a grid for the chip, the loop strides over the slots
    hipLaunchKernelGGL(k_degree_count, dim3(256u * 16u), dim3(256), 0, stream, rowptr, col, erow, (int)N, (unsigned *)degree);
    if (keys)
        hipLaunchKernelGGL(k_degree_keys, dim3(capped_grid((size_t)N, 256)), dim3(256), 0, stream, (const long long *)degree, (int)N,
                           (u64 *)keys);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" int pope_topk_max_k(void) { return POPE_TOPK_MAX_K; }

extern "C" size_t pope_topk_scratch_bytes(int64_t N, int64_t K) { return topk_sizes_ok(N, K) ? topk_layout((size_t)N).total : 0; }

extern "C" int pope_topk_u64(const uint64_t *keys, int64_t N, int64_t K, uint64_t *out, void *scratch, size_t scratch_bytes,
                             void *stream_) {
    clear_error();
    POPE_REQUIRE(N > 0 && N < INT32_MAX, "pope_topk_u64: need 0 < N < 2^31 (N=%lld)", (long long)N);
    POPE_REQUIRE(K >= 1 && K <= N && K <= POPE_TOPK_MAX_K, "pope_topk_u64: need 1 <= K <= min(N, %d) (K=%lld N=%lld)", POPE_TOPK_MAX_K,
                 (long long)K, (long long)N);
    POPE_REQUIRE(keys && out && scratch, "pope_topk_u64: null pointer");
    const TopkScratch L = topk_layout((size_t)N);
    if (scratch_bytes < L.total) {
        set_error("pope_topk_u64: scratch %zu < %zu bytes", scratch_bytes, L.total);
        return POPE_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)scratch;
    TopkCtl *ctl = (TopkCtl *)(base + L.ctl);
    unsigned *hist = (unsigned *)(base + L.hist);
    u64 *cand = (u64 *)(base + L.cand);
    const u64 *in = (const u64 *)keys;
    u64 *res = (u64 *)out;
    const unsigned n = (unsigned)N, k = (unsigned)K;
    POPE_HIP(hipMemsetAsync(base, 0, L.cand, stream));            // the control block and the eight histograms
    // the candidates of launch D >= 2 are known on the device only: the grid is sized for N, surplus blocks narrow and leave
    const unsigned grid = capped_grid((size_t)N, TOPK_BLOCK, TOPK_GRID_CAP);
    topk_launch<0>(grid, stream, in, n, k, ctl, hist, cand, res);
    topk_launch<1>(grid, stream, in, n, k, ctl, hist, cand, res);
    topk_launch<2>(grid, stream, in, n, k, ctl, hist, cand, res);
    topk_launch<3>(grid, stream, in, n, k, ctl, hist, cand, res);
    topk_launch<4>(grid, stream, in, n, k, ctl, hist, cand, res);
    topk_launch<5>(grid, stream, in, n, k, ctl, hist, cand, res);
    topk_launch<6>(grid, stream, in, n, k, ctl, hist, cand, res);
    topk_launch<7>(grid, stream, in, n, k, ctl, hist, cand, res);
    topk_launch<8>(grid, stream, in, n, k, ctl, hist, cand, res);
    int p = 1;
    while (p < (int)K) p <<= 1;
    hipLaunchKernelGGL(k_topk_sort, dim3(1), dim3(TOPK_SORT_THREADS), 0, stream, res, (int)K, p);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}
