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
//
// 3. pope_topk_f64: the same select over the pairs (score[v], v) for the other five biased methods (/root/reference/utils.py:26-30
//    pagerank, :32-36 betweenness, :44-48 eigenvector, :50-54 closeness, :56-60 clustering: each ends in the ascending stable sort
//    of its float64 scores and the slice that keeps the last K, utils.py:29-30 and the same two lines of every method).  The pass
//    kernel is ONE template over the key: TopkU64 (8 digits, the caller's keys) and TopkF64 (12 digits: the 8 of score_key(score),
//    NumPy's sort order as an unsigned integer, then the 4 of the node id).  All 96-bit keys are distinct, so "stable sort, last
//    K" is "the K largest pairs, ascending": ties go to the higher node ids, in ascending id order.  Launch 0 reads the doubles
//    and forms the keys on the fly (node = index): no array of N keys exists.  Candidates and the K selected pairs live in the
//    scratch as separate key and node arrays; a digit that narrows nothing still copies nothing, which is what a tie class does
//    to the score digits of the survivors.  After digit 11 the prefix is the K-th largest pair itself.  A one-block bitonic
//    sort over K (key, node) pairs in LDS writes the node ids and, if asked, scores[node] (the stored double, not the key).
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
// The order-preserving 64-bit key of a float64 score, NumPy's sort order: -0.0 == +0.0, every NaN equal to every other NaN and
// above +inf.  Unsigned comparison of the keys is that order.
__host__ __device__ inline u64 score_key(double score) {
    u64 b;
    __builtin_memcpy(&b, &score, sizeof b);
    const u64 mag = b & 0x7FFFFFFFFFFFFFFFull;
    if (mag == 0ull) return 0x8000000000000000ull;               // +-0.0
    if (mag > 0x7FF0000000000000ull) return ~0ull;               // NaN, any sign and payload
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}

// The two key widths of the select.  A trait names the key, where launch 0 finds it, the buffers that hold candidates and
// results, and the digits (most significant first).
struct TopkU64 {                      // pope_topk_u64: the caller's 64-bit keys, 8 digits
    typedef u64 Key;
    typedef const u64 *Src;
    struct Buf { u64 *p; };
    static constexpr int DIGITS = 8;
    static __device__ __forceinline__ Key zero() { return 0ull; }
    static __device__ __forceinline__ Key load_src(Src s, size_t i) { return s[i]; }
    static __device__ __forceinline__ Key load(Buf b, size_t i) { return b.p[i]; }
    static __device__ __forceinline__ void store(Buf b, size_t i, Key k) { b.p[i] = k; }
    static __device__ __forceinline__ Buf at(Buf b, size_t off) { return Buf{b.p + off}; }
    template <int DG> static __device__ __forceinline__ unsigned digit(Key k) { return (unsigned)(k >> (56 - 8 * DG)) & 255u; }
    template <int DG> static __device__ __forceinline__ Key with_digit(Key prefix, unsigned bin) { return prefix | ((u64)bin << (56 - 8 * DG)); }
};

struct ScoreNode {                    // the 96-bit key (score_key(score[v]), v): all keys of a call are distinct
    u64 s;
    unsigned v;
};

struct TopkF64 {                      // pope_topk_f64: pairs (score, node), 8 score digits then 4 node digits
    typedef ScoreNode Key;
    typedef const double *Src;
    struct Buf { u64 *s; unsigned *v; };                          // keys and nodes in separate arrays
    static constexpr int DIGITS = 12;
    static __device__ __forceinline__ Key zero() { return Key{0ull, 0u}; }
    static __device__ __forceinline__ Key load_src(Src s, size_t i) { return Key{score_key(s[i]), (unsigned)i}; }   // launch 0 forms the keys: node = index
    static __device__ __forceinline__ Key load(Buf b, size_t i) { return Key{b.s[i], b.v[i]}; }
    static __device__ __forceinline__ void store(Buf b, size_t i, Key k) { b.s[i] = k.s; b.v[i] = k.v; }
    static __device__ __forceinline__ Buf at(Buf b, size_t off) { return Buf{b.s + off, b.v + off}; }
    template <int DG> static __device__ __forceinline__ unsigned digit(Key k) {
        if constexpr (DG < 8) return (unsigned)(k.s >> (56 - 8 * DG)) & 255u;
        else return (k.v >> (24 - 8 * (DG - 8))) & 255u;
    }
    template <int DG> static __device__ __forceinline__ Key with_digit(Key prefix, unsigned bin) {
        if constexpr (DG < 8) prefix.s |= (u64)bin << (56 - 8 * DG);
        else prefix.v |= bin << (24 - 8 * (DG - 8));
        return prefix;
    }
};

template <class T>
struct TopkState {                    // after D digits:
    typename T::Key prefix;           // the top D digits of the K-th largest key (lower digits zero)
    unsigned remaining;               // how many keys with that prefix are still to take (>= 1)
    unsigned n;                       // how many keys have that prefix = the candidates the next launch reads ...
    unsigned src;                     // ... from here: 0 = the caller's keys / scores, 1 / 2 = a candidate buffer
};

template <class T>
struct TopkCtl {
    TopkState<T> st[T::DIGITS + 1];   // st[D] for D = 1 .. DIGITS (st[0] = {0, K, N, 0} comes from the arguments)
    unsigned cursor[T::DIGITS + 1];   // candidates written by launch D
    unsigned emitted;                 // keys written to the result so far
};

struct TopkScratch {
    size_t ctl, hist, cand, cand_nodes, res, res_nodes, total;
};

template <class T>
__host__ __device__ inline TopkScratch topk_layout(size_t N, size_t K) {
    constexpr bool pairs = T::DIGITS > 8;
    TopkScratch L;
    size_t o = 0;
    L.ctl = o;  o += (sizeof(TopkCtl<T>) + 255) / 256 * 256;
    L.hist = o; o += (size_t)T::DIGITS * 256 * sizeof(unsigned);
    L.cand = o; o += (2 * N * sizeof(u64) + 255) / 256 * 256;     // two candidate buffers, read one / write the other
    L.cand_nodes = o;
    if (pairs) o += (2 * N * sizeof(unsigned) + 255) / 256 * 256; // ... and the nodes that go with them
    L.res = o;
    if (pairs) o += (K * sizeof(u64) + 255) / 256 * 256;          // the K selected pairs before the sort (u64: the caller's out)
    L.res_nodes = o;
    if (pairs) o += (K * sizeof(unsigned) + 255) / 256 * 256;
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

template <class T, int D>
__global__ __launch_bounds__(TOPK_BLOCK) void k_topk_pass(typename T::Src keys, unsigned N, unsigned K, TopkCtl<T> *__restrict__ ctl,
                                                          unsigned *__restrict__ hist, typename T::Buf cand, typename T::Buf out) {
    typedef typename T::Key Key;
    constexpr int LAST = T::DIGITS;                               // launch LAST reads the last digit and fills the tail
    __shared__ unsigned h[256];
    __shared__ unsigned sel[2];
    const int t = threadIdx.x, lane = t & 63;
    TopkState<T> prev = {T::zero(), K, N, 0u}, cur = prev;
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
        cur.prefix = T::template with_digit<D - 1>(prev.prefix, bin);
        cur.remaining = prev.remaining - sel[1];
        cur.n = h[bin];
        cur.src = prev.src;
        if constexpr (D < LAST) {
            // a digit that narrows nothing (the high digits of small keys, runs of equal keys, the score digits of a tie class)
            // keeps the candidates where they are: the next launch reads the same buffer again and no wave queues at the cursor
            copy = cur.n != prev.n;
            if (copy) cur.src = prev.src == 1u ? 2u : 1u;
        }
        if (blockIdx.x == 0 && t == 0) ctl->st[D] = cur;
        __syncthreads();
    }
    h[t] = 0;
    __syncthreads();
    const typename T::Buf from = T::at(cand, (size_t)(prev.src == 2u ? 1u : 0u) * N);   // read only if prev.src != 0
    const typename T::Buf dst = T::at(cand, (size_t)(cur.src == 2u ? 1u : 0u) * N);      // written only if `copy`
    const size_t n = prev.n < N ? prev.n : N;                     // D <= 1: N
    for (size_t base = (size_t)blockIdx.x * TOPK_BLOCK; base < n; base += (size_t)gridDim.x * TOPK_BLOCK) {   // whole waves enter
        const size_t i = base + t;
        const bool valid = i < n;
        Key key = T::zero();
        if (valid) key = prev.src == 0u ? T::load_src(keys, i) : T::load(from, i);
        bool keep = valid;
        if constexpr (D >= 1) {
            const unsigned dp = T::template digit<D - 1>(key);
            const bool emit = valid && dp > bin;
            keep = valid && dp == bin;
            const unsigned long long em = __ballot(emit);
            if (em) {
                const unsigned pos = wave_slot(em, &ctl->emitted, lane);
                if (emit && pos < K) T::store(out, pos, key);
            }
        }
        if constexpr (D < LAST) {
            const unsigned long long km = __ballot(keep);
            if (km) {
                if (copy) {
                    const unsigned pos = wave_slot(km, &ctl->cursor[D], lane);
                    if (keep && pos < N) T::store(dst, pos, key);
                }
                const unsigned dg = T::template digit<D>(key);
                const unsigned d0 = (unsigned)__shfl((int)dg, __ffsll((long long)km) - 1, 64);
                if (__ballot(keep && dg == d0) == km) {           // the whole wave in one bin (the high digits of small keys)
                    if (lane == __ffsll((long long)km) - 1) atomicAdd(&h[d0], (unsigned)__popcll(km));
                } else if (keep) {
                    atomicAdd(&h[dg], 1u);
                }
            }
        }
    }
    if constexpr (D < LAST) {
        __syncthreads();
        const unsigned c = h[t];
        if (c) atomicAdd(&hist[D * 256 + t], c);
    }
    if (D == LAST && blockIdx.x == 0)                             // the copies of T itself: the result's tail (pairs: the one pair)
        for (unsigned i = t; i < cur.remaining; i += TOPK_BLOCK) T::store(out, K - cur.remaining + i, cur.prefix);   // remaining <= K
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

// The same sort over K pairs (score key, node), keys and nodes in separate LDS arrays (48 KB at POPE_TOPK_MAX_K); the pads
// (~0, ~0) lie above every real pair (node < 2^31).  Writes the node ids and, if asked, the scores THEY HAVE IN `scores` (the key
// has forgotten the sign of a zero and a NaN's payload).
__global__ __launch_bounds__(TOPK_SORT_THREADS) void k_topk_sort_pairs(const u64 *__restrict__ res, const unsigned *__restrict__ res_nodes,
                                                                       const double *__restrict__ scores, unsigned N, int K, int P,
                                                                       long long *__restrict__ nodes_out, double *__restrict__ scores_out) {
    __shared__ u64 s[POPE_TOPK_MAX_K];
    __shared__ unsigned v[POPE_TOPK_MAX_K];
    const int t = threadIdx.x;
    for (int i = t; i < P; i += TOPK_SORT_THREADS) {
        s[i] = i < K ? res[i] : ~0ull;
        v[i] = i < K ? res_nodes[i] : ~0u;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += TOPK_SORT_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const u64 a = s[i], b = s[x];
                    const unsigned va = v[i], vb = v[x];
                    if ((a > b || (a == b && va > vb)) == ((i & k) == 0)) {
                        s[i] = b;
                        s[x] = a;
                        v[i] = vb;
                        v[x] = va;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = t; i < K; i += TOPK_SORT_THREADS) {
        const unsigned node = v[i] < N ? v[i] : N - 1u;           // always < N: a node is an index of `scores`
        nodes_out[i] = (long long)node;
        if (scores_out) scores_out[i] = scores[node];
    }
}

}  // namespace pope

using namespace pope;

static_assert((POPE_TOPK_MAX_K & (POPE_TOPK_MAX_K - 1)) == 0 && POPE_TOPK_MAX_K >= 1024 &&
                  POPE_TOPK_MAX_K * (sizeof(u64) + sizeof(unsigned)) <= 64 * 1024,
              "POPE_TOPK_MAX_K: a power of two that the one-block LDS sorts hold (keys, and keys + nodes)");

namespace {

bool topk_sizes_ok(int64_t N, int64_t K) { return N > 0 && N < INT32_MAX && K >= 1 && K <= N && K <= POPE_TOPK_MAX_K; }

template <class T>
struct TopkArgs {
    typename T::Src keys;
    unsigned N, K;
    TopkCtl<T> *ctl;
    unsigned *hist;
    typename T::Buf cand, out;
    unsigned grid;
    hipStream_t stream;
};

// launches 0 .. DIGITS, one per digit boundary
template <class T, int D = 0>
void topk_passes(const TopkArgs<T> &a) {
    hipLaunchKernelGGL((k_topk_pass<T, D>), dim3(a.grid), dim3(TOPK_BLOCK), 0, a.stream, a.keys, a.N, a.K, a.ctl, a.hist, a.cand, a.out);
    if constexpr (D < T::DIGITS) topk_passes<T, D + 1>(a);
}

int sort_width(int64_t K) {
    int p = 1;
    while (p < (int)K) p <<= 1;
    return p;
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

extern "C" size_t pope_topk_scratch_bytes(int64_t N, int64_t K) {
    return topk_sizes_ok(N, K) ? topk_layout<TopkU64>((size_t)N, (size_t)K).total : 0;
}

extern "C" int pope_topk_u64(const uint64_t *keys, int64_t N, int64_t K, uint64_t *out, void *scratch, size_t scratch_bytes,
                             void *stream_) {
    clear_error();
    POPE_REQUIRE(N > 0 && N < INT32_MAX, "pope_topk_u64: need 0 < N < 2^31 (N=%lld)", (long long)N);
    POPE_REQUIRE(K >= 1 && K <= N && K <= POPE_TOPK_MAX_K, "pope_topk_u64: need 1 <= K <= min(N, %d) (K=%lld N=%lld)", POPE_TOPK_MAX_K,
                 (long long)K, (long long)N);
    POPE_REQUIRE(keys && out && scratch, "pope_topk_u64: null pointer");
    const TopkScratch L = topk_layout<TopkU64>((size_t)N, (size_t)K);
    if (scratch_bytes < L.total) {
        set_error("pope_topk_u64: scratch %zu < %zu bytes", scratch_bytes, L.total);
        return POPE_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)scratch;
    u64 *res = (u64 *)out;
    POPE_HIP(hipMemsetAsync(base, 0, L.cand, stream));            // the control block and the eight histograms
    // the candidates of launch D >= 2 are known on the device only: the grid is sized for N, surplus blocks narrow and leave
    TopkArgs<TopkU64> a = {(const u64 *)keys, (unsigned)N, (unsigned)K, (TopkCtl<TopkU64> *)(base + L.ctl), (unsigned *)(base + L.hist),
                           TopkU64::Buf{(u64 *)(base + L.cand)}, TopkU64::Buf{res}, capped_grid((size_t)N, TOPK_BLOCK, TOPK_GRID_CAP),
                           stream};
    topk_passes(a);
    hipLaunchKernelGGL(k_topk_sort, dim3(1), dim3(TOPK_SORT_THREADS), 0, stream, res, (int)K, sort_width(K));
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" size_t pope_topk_f64_scratch_bytes(int64_t N, int64_t K) {
    return topk_sizes_ok(N, K) ? topk_layout<TopkF64>((size_t)N, (size_t)K).total : 0;
}

extern "C" int pope_topk_f64(const double *scores, int64_t N, int64_t K, int64_t *nodes_out, double *scores_out, void *scratch,
                             size_t scratch_bytes, void *stream_) {
    clear_error();
    POPE_REQUIRE(N > 0 && N < INT32_MAX, "pope_topk_f64: need 0 < N < 2^31 (N=%lld)", (long long)N);
    POPE_REQUIRE(K >= 1 && K <= N && K <= POPE_TOPK_MAX_K, "pope_topk_f64: need 1 <= K <= min(N, %d) (K=%lld N=%lld)", POPE_TOPK_MAX_K,
                 (long long)K, (long long)N);
    POPE_REQUIRE(scores && nodes_out && scratch, "pope_topk_f64: null pointer");
    const TopkScratch L = topk_layout<TopkF64>((size_t)N, (size_t)K);
    if (scratch_bytes < L.total) {
        set_error("pope_topk_f64: scratch %zu < %zu bytes", scratch_bytes, L.total);
        return POPE_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    char *base = (char *)scratch;
    POPE_HIP(hipMemsetAsync(base, 0, L.cand, stream));            // the control block and the twelve histograms
    const TopkF64::Buf res = {(u64 *)(base + L.res), (unsigned *)(base + L.res_nodes)};   // every slot is written before the sort reads it
    TopkArgs<TopkF64> a = {scores, (unsigned)N, (unsigned)K, (TopkCtl<TopkF64> *)(base + L.ctl), (unsigned *)(base + L.hist),
                           TopkF64::Buf{(u64 *)(base + L.cand), (unsigned *)(base + L.cand_nodes)}, res,
                           capped_grid((size_t)N, TOPK_BLOCK, TOPK_GRID_CAP), stream};
    topk_passes(a);
    hipLaunchKernelGGL(k_topk_sort_pairs, dim3(1), dim3(TOPK_SORT_THREADS), 0, stream, (const u64 *)res.s, (const unsigned *)res.v, scores,
                       (unsigned)N, (int)K, sort_width(K), (long long *)nodes_out, scores_out);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" int pope_score_keys_host(const double *scores, int64_t n, uint64_t *keys) {
    clear_error();
    POPE_REQUIRE(n >= 0, "pope_score_keys_host: need n >= 0 (n=%lld)", (long long)n);
    POPE_REQUIRE(n == 0 || (scores && keys), "pope_score_keys_host: null pointer");
    for (int64_t i = 0; i < n; ++i) keys[i] = score_key(scores[i]);   // the function the kernels call, compiled for the host
    return POPE_OK;
}
