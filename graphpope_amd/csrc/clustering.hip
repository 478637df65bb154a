// Biased anchor selection on the device: the integers behind nx.clustering for sampling_method='clustering_coefficient'.
//
// Replaces /root/reference/utils.py:56-60  nx.clustering(to_networkx(data)).  On the DiGraph (NetworkX 3.4.2,
// cluster._directed_triangles_and_degree_iter, unweighted) with A = its adjacency without self-loops and M = A + A^T
// (symmetric, zero diagonal, entries 0 / 1 / 2), node i gets
//     T_i = (M^3)_ii,   dt_i = sum_k M_ik,   db_i = #{k : M_ik = 2},
//     c_i = 0 if T_i == 0 else T_i / ((dt_i (dt_i - 1) - 2 db_i) * 2)     (the host evaluates this line).
// Exact integers, so the scores are NetworkX's bit for bit.
//
// 1. M from the two canonical CSRs (pope_csr_build_canonical of edge_index and of its flip: rows sorted, repeats
//    adjacent).  Every slot of both is one candidate neighbour; a slot is kept if it starts its run and is no self-loop,
//    and a predecessor slot only if the node is not also a successor (that one carries weight 2).  One code byte per
//    slot, an exclusive scan of (weight << 32 | 1), and each row's distinct degree, dt and db are differences of the scan.
// 2. Orientation by the total order (distinct degree, id): N+(i) = the neighbours after i.  A second scan places the
//    kept slots, a rocPRIM segmented sort orders every row; an entry is (k << 1 | [M_ik == 2]).
// 3. Triangles: one wave64 per row i stages N+(i) in LDS (CL_CAP entries at a time), walks N+(j) of every j in N+(i)
//    load-balanced over the lanes, and looks each k up by binary search.  A triangle i < j < k of weight
//    w = M_ij M_ik M_jk is found exactly once and adds 2w to T_i (registers), T_j and T_k (LDS accumulators of the
//    staged row, flushed with one 64-bit integer atomic per node and row).  Integer sums: exact, any run order.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "common.h"
#include "wave.h"

namespace pope {

constexpr int CL_CAP = 1024;         // entries of N+(i) staged per chunk: rows beyond it run in several chunks
constexpr int CL_WAVES = 4;          // waves (rows in flight) per 256-thread block

// First position in the sorted run a[beg, end) whose value is >= v.
__device__ __forceinline__ int lower_bound_i32(const int *__restrict__ a, int beg, int end, int v) {
    while (beg < end) {
        const int mid = beg + ((end - beg) >> 1);
        if (a[mid] < v) beg = mid + 1;
        else end = mid;
    }
    return beg;
}

// code[s] for the 2E candidate slots: s < E the successor slot s of the CSR by source, s >= E the predecessor slot s - E
// of the CSR by target.  0 = dropped, 1 or 2 = kept with that weight.  code[2E] = 0 pads the scans to 2E + 1.
__global__ __launch_bounds__(256) void k_cl_codes(const int *__restrict__ rp_s, const int *__restrict__ col_s, const int *__restrict__ row_s,
                                                  const int *__restrict__ rp_t, const int *__restrict__ col_t, const int *__restrict__ row_t,
                                                  int E, unsigned char *__restrict__ code) {
    const size_t slots = 2 * (size_t)E;                          // <= 2^31 - 2: the stride below must not wrap an int
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s <= slots; s += (size_t)gridDim.x * blockDim.x) {
        unsigned char c = 0;
        if (s < slots) {
            const bool fwd = s < (size_t)E;
            const int p = (int)(fwd ? s : s - E);
            const int *rp = fwd ? rp_s : rp_t, *col = fwd ? col_s : col_t;
            const int *orp = fwd ? rp_t : rp_s, *ocol = fwd ? col_t : col_s;
            const int i = (fwd ? row_s : row_t)[p], v = col[p];
            if (v != i && (p == rp[i] || col[p - 1] != v)) {
                const int oe = orp[i + 1], q = lower_bound_i32(ocol, orp[i], oe, v);
                const bool both = q < oe && ocol[q] == v;
                c = fwd ? (both ? 2 : 1) : (both ? 0 : 1);
            }
        }
        code[s] = c;
    }
}

struct CountWeight {                 // kept slot -> (weight << 32) | 1: one scan gives the distinct count and the sum of weights
    __host__ __device__ u64 operator()(unsigned char c) const { return c ? ((u64)c << 32) | 1ull : 0ull; }
};

struct Kept {
    __host__ __device__ int operator()(unsigned char c) const { return c != 0; }
};

// Row i: distinct degree d (low halves of the scan), dt (high halves), db = dt - d.
__global__ __launch_bounds__(256) void k_cl_degrees(const int *__restrict__ rp_s, const int *__restrict__ rp_t, int N, int E,
                                                    const u64 *__restrict__ x, int *__restrict__ deg, long long *__restrict__ dt,
                                                    long long *__restrict__ db) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        const u64 a = x[rp_s[i]], b = x[rp_s[i + 1]], c = x[(size_t)E + rp_t[i]], d = x[(size_t)E + rp_t[i + 1]];
        const long long cnt = (long long)((unsigned)b - (unsigned)a) + (long long)((unsigned)d - (unsigned)c);
        const long long w = (long long)((b >> 32) - (a >> 32)) + (long long)((d >> 32) - (c >> 32));
        deg[i] = (int)cnt;
        dt[i] = w;
        db[i] = w - cnt;
    }
}

// Keep a slot's code only if its node comes after the row's node in the order (distinct degree, id).
__global__ __launch_bounds__(256) void k_cl_orient(const int *__restrict__ col_s, const int *__restrict__ row_s, const int *__restrict__ col_t,
                                                   const int *__restrict__ row_t, int E, const int *__restrict__ deg,
                                                   unsigned char *__restrict__ code) {
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < 2 * (size_t)E; s += (size_t)gridDim.x * blockDim.x) {
        const unsigned char c = code[s];
        if (!c) continue;
        const bool fwd = s < (size_t)E;
        const int p = (int)(fwd ? s : s - E);
        const int i = (fwd ? row_s : row_t)[p], v = (fwd ? col_s : col_t)[p];
        const int di = deg[i], dv = deg[v];
        if (!(dv > di || (dv == di && v > i))) code[s] = 0;
    }
}

// Oriented row i = its kept successor slots, then its kept predecessor slots: offsets from the scan y of the kept flags.
// y runs over both halves, so the predecessor half's count before row i is y[E + rp_t[i]] - y[E]: rp_o[0] = 0 and
// rp_o[N] = y[2E] = the kept pairs (at most E, the room the layout gives the oriented rows).
__global__ __launch_bounds__(256) void k_cl_rowptr(const int *__restrict__ rp_s, const int *__restrict__ rp_t, int N, int E,
                                                   const int *__restrict__ y, int *__restrict__ rp_o) {
    const int succ_total = y[E];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= N; i += gridDim.x * blockDim.x)
        rp_o[i] = y[rp_s[i]] + (y[(size_t)E + rp_t[i]] - succ_total);
}

__global__ __launch_bounds__(256) void k_cl_fill(const int *__restrict__ rp_s, const int *__restrict__ col_s, const int *__restrict__ row_s,
                                                 const int *__restrict__ rp_t, const int *__restrict__ col_t, const int *__restrict__ row_t,
                                                 int E, const unsigned char *__restrict__ code, const int *__restrict__ y,
                                                 const int *__restrict__ rp_o, unsigned *__restrict__ out) {
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < 2 * (size_t)E; s += (size_t)gridDim.x * blockDim.x) {
        const unsigned char c = code[s];
        if (!c) continue;
        const bool fwd = s < (size_t)E;
        const int p = (int)(fwd ? s : s - E);
        const int i = (fwd ? row_s : row_t)[p], v = (fwd ? col_s : col_t)[p];
        const int pos = fwd ? rp_o[i] + y[p] - y[rp_s[i]]
                            : rp_o[i] + (y[rp_s[i + 1]] - y[rp_s[i]]) + y[(size_t)E + p] - y[(size_t)E + rp_t[i]];
        out[pos] = ((unsigned)v << 1) | (c == 2 ? 1u : 0u);
    }
}

// LDS image of one wave: the staged chunk of N+(i) with its accumulators, and the batch of (up to) 64 j's being walked.
struct ClWave {
    unsigned key[CL_CAP];            // k << 1 | [M_ik == 2], ascending
    unsigned acc[CL_CAP];            // 2w added to T_k / T_j for the staged k (or j) during this row
    int pre[64];                     // inclusive prefix of |N+(j)| over the batch
    int start[64];                   // rowptr of j
    unsigned jkey[64];               // j << 1 | [M_ij == 2]
    unsigned accj[64];               // 2w added to T_j of batch lane s during this batch
};

__device__ __forceinline__ void wave_lds_sync() {
    // A wave's LDS instructions execute in order; this only keeps the compiler from moving LDS accesses across it.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void k_cl_triangles(const int *__restrict__ rp_o, const unsigned *__restrict__ nbr, int N,
                                                      unsigned long long *__restrict__ T) {
    __shared__ ClWave lds[CL_WAVES];
    const int lane = threadIdx.x & 63;
    ClWave &L = lds[threadIdx.x >> 6];
    for (int i = blockIdx.x * CL_WAVES + (threadIdx.x >> 6); i < N; i += gridDim.x * CL_WAVES) {
        const int base = rp_o[i], deg = rp_o[i + 1] - base;
        if (deg < 2) continue;                                    // i is the lowest node of its triangles: needs two out-neighbours
        unsigned long long ti = 0;
        for (int c0 = 0; c0 < deg; c0 += CL_CAP) {
            const int nc = min(CL_CAP, deg - c0);
            for (int t = lane; t < nc; t += 64) {
                L.key[t] = nbr[base + c0 + t];
                L.acc[t] = 0;
            }
            wave_lds_sync();
            const unsigned kmin = L.key[0] & ~1u, kmax = L.key[nc - 1] | 1u;
            for (int j0 = 0; j0 < deg; j0 += 64) {
                const int jj = j0 + lane;
                unsigned jk = 0;
                int st = 0, len = 0;
                if (jj < deg) {
                    jk = nbr[base + jj];
                    const int j = (int)(jk >> 1);
                    st = rp_o[j];
                    len = rp_o[j + 1] - st;
                }
                const int inc = wave_inclusive_scan(len, lane);
                const int total = __shfl(inc, 63, 64);
                L.pre[lane] = inc;
                L.start[lane] = st;
                L.jkey[lane] = jk;
                L.accj[lane] = 0;
                wave_lds_sync();
                for (int t = lane; t < total; t += 64) {
                    int s = 0;                                    // the batch lane whose list holds item t: first pre[s] > t
#pragma unroll
                    for (int half = 32; half >= 1; half >>= 1)
                        if (L.pre[s + half - 1] <= t) s += half;
                    const int off = t - (s ? L.pre[s - 1] : 0);
                    const unsigned kk = nbr[L.start[s] + off];
                    if (kk < kmin || kk > kmax) continue;
                    int lo = 0, hi = nc;                          // lower bound of k << 1 in the staged chunk
                    const unsigned kx = kk & ~1u;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (L.key[mid] < kx) lo = mid + 1;
                        else hi = mid;
                    }
                    if (lo == nc || (L.key[lo] >> 1) != (kk >> 1)) continue;
                    const unsigned w2 = 2u * (1u + (L.jkey[s] & 1u)) * (1u + (L.key[lo] & 1u)) * (1u + (kk & 1u));
                    ti += w2;
                    atomicAdd(&L.acc[lo], w2);
                    atomicAdd(&L.accj[s], w2);
                }
                wave_lds_sync();
                const unsigned aj = L.accj[lane];
                if (aj) {                                         // j in the staged chunk: its accumulator; otherwise straight out
                    if (jj >= c0 && jj < c0 + nc) atomicAdd(&L.acc[jj - c0], aj);
                    else atomicAdd(&T[jk >> 1], (unsigned long long)aj);
                }
                wave_lds_sync();
            }
            for (int t = lane; t < nc; t += 64) {
                const unsigned a = L.acc[t];
                if (a) atomicAdd(&T[L.key[t] >> 1], (unsigned long long)a);
            }
            wave_lds_sync();
        }
        ti = wave_sum(ti);
        if (lane == 0 && ti) atomicAdd(&T[i], ti);
    }
}

}  // namespace pope

using namespace pope;

namespace {

struct ClScratch {
    size_t code, x, deg, rp_o, nbr_u, nbr, scan_tmp, sort_tmp, total;
    size_t scan_bytes, sort_bytes;   // rocPRIM's temp sizes for this device
    hipError_t err;                  // a failed rocPRIM size query (no device visible): the layout is unknown
};

hipError_t cl_scan_bytes(size_t n, size_t *bytes) {
    size_t a = 0, b = 0;
    const unsigned char *c = nullptr;
    hipError_t e = rocprim::exclusive_scan(nullptr, a, rocprim::make_transform_iterator(c, CountWeight()), (u64 *)nullptr, 0ull, n,
                                           rocprim::plus<u64>());
    if (e == hipSuccess)
        e = rocprim::exclusive_scan(nullptr, b, rocprim::make_transform_iterator(c, Kept()), (int *)nullptr, 0, n, rocprim::plus<int>());
    *bytes = a > b ? a : b;
    return e;
}

hipError_t cl_sort_bytes(size_t E, size_t N, size_t *bytes) {
    *bytes = 0;
    return rocprim::segmented_radix_sort_keys(nullptr, *bytes, (const unsigned *)nullptr, (unsigned *)nullptr, (unsigned)E, (unsigned)N,
                                              (const int *)nullptr, (const int *)nullptr);
}

// code [2E + 1] B | scan x [2E + 1] u64 (the second scan, int [2E + 1], reuses it) | deg [N] | oriented rowptr [N + 1] |
// oriented entries [E] unsorted, [E] sorted (an oriented row holds each unordered pair once: rowptr[N] = pairs <= E) | temps
ClScratch cl_layout(int64_t N, int64_t E) {
    ClScratch L;
    const size_t slots = (size_t)(2 * E + 1), e = (size_t)(E > 0 ? E : 1);
    L.err = cl_scan_bytes(slots, &L.scan_bytes);
    if (L.err == hipSuccess) L.err = cl_sort_bytes(e, (size_t)N, &L.sort_bytes);
    size_t o = 0;
    L.code = o;     o += align_up(slots, 256);
    L.x = o;        o += align_up(slots * sizeof(u64), 256);
    L.deg = o;      o += align_up((size_t)N * sizeof(int), 256);
    L.rp_o = o;     o += align_up((size_t)(N + 1) * sizeof(int), 256);
    L.nbr_u = o;    o += align_up(e * sizeof(unsigned), 256);
    L.nbr = o;      o += align_up(e * sizeof(unsigned), 256);
    L.scan_tmp = o; o += align_up(L.scan_bytes, 256);
    L.sort_tmp = o; o += align_up(L.sort_bytes, 256);
    L.total = o;
    return L;
}

bool cl_sizes_ok(int64_t N, int64_t E) { return N > 0 && N < INT32_MAX && E >= 0 && E <= (INT32_MAX - 1) / 2; }

}  // namespace

extern "C" size_t pope_clustering_scratch_bytes(int64_t N, int64_t E) {
    if (!cl_sizes_ok(N, E)) return 0;
    const ClScratch L = cl_layout(N, E);
    return L.err == hipSuccess ? L.total : 0;
}

extern "C" int pope_clustering_counts(const int32_t *rowptr, const int32_t *col, const int32_t *erow, const int32_t *rowptr_by_target,
                                      const int32_t *sources, const int32_t *erow_by_target, int64_t N, int64_t E, int64_t *T,
                                      int64_t *dt, int64_t *db, void *scratch, size_t scratch_bytes, void *stream_) {
    clear_error();
    POPE_REQUIRE(N > 0 && N < INT32_MAX && E >= 0, "pope_clustering_counts: need 0 < N < 2^31 and E >= 0 (N=%lld E=%lld)",
                 (long long)N, (long long)E);
    POPE_REQUIRE(E <= (INT32_MAX - 1) / 2, "pope_clustering_counts: 2 * E = %lld slots of M do not fit int32 offsets", 2 * (long long)E);
    POPE_REQUIRE(rowptr && rowptr_by_target && T && dt && db && scratch &&
                     ((col && erow && sources && erow_by_target) || E == 0),
                 "pope_clustering_counts: null pointer");
    const ClScratch L = cl_layout(N, E);
    if (L.err != hipSuccess) {
        set_error("pope_clustering_counts: rocPRIM temp-size query failed: %s", hipGetErrorString(L.err));
        return POPE_ERR_HIP;
    }
    if (scratch_bytes < L.total) {
        set_error("pope_clustering_counts: scratch %zu < %zu bytes", scratch_bytes, L.total);
        return POPE_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const int n = (int)N, e = (int)E;
    POPE_HIP(hipMemsetAsync(T, 0, (size_t)N * sizeof(int64_t), stream));
    if (E == 0) {
        POPE_HIP(hipMemsetAsync(dt, 0, (size_t)N * sizeof(int64_t), stream));
        POPE_HIP(hipMemsetAsync(db, 0, (size_t)N * sizeof(int64_t), stream));
        return POPE_OK;
    }
    char *base = (char *)scratch;
    unsigned char *code = (unsigned char *)(base + L.code);
    u64 *x = (u64 *)(base + L.x);
    int *y = (int *)(base + L.x);                                  // the second scan: x is dead once the degrees are out
    int *deg = (int *)(base + L.deg), *rp_o = (int *)(base + L.rp_o);
    unsigned *nbr_u = (unsigned *)(base + L.nbr_u), *nbr = (unsigned *)(base + L.nbr);
    void *scan_tmp = base + L.scan_tmp, *sort_tmp = base + L.sort_tmp;
    const size_t slots = (size_t)(2 * E + 1);
    size_t scan_bytes = L.scan_bytes, sort_bytes = L.sort_bytes;

    hipLaunchKernelGGL(k_cl_codes, dim3(capped_grid(slots, 256)), dim3(256), 0, stream, rowptr, col, erow, rowptr_by_target, sources,
                       erow_by_target, e, code);
    POPE_HIP(rocprim::exclusive_scan(scan_tmp, scan_bytes, rocprim::make_transform_iterator((const unsigned char *)code, CountWeight()), x,
                                     0ull, slots, rocprim::plus<u64>(), stream));
    hipLaunchKernelGGL(k_cl_degrees, dim3(capped_grid((size_t)N, 256)), dim3(256), 0, stream, rowptr, rowptr_by_target, n, e, x, deg,
                       (long long *)dt, (long long *)db);
    hipLaunchKernelGGL(k_cl_orient, dim3(capped_grid(slots, 256)), dim3(256), 0, stream, col, erow, sources, erow_by_target, e, deg, code);
    POPE_HIP(rocprim::exclusive_scan(scan_tmp, scan_bytes, rocprim::make_transform_iterator((const unsigned char *)code, Kept()), y, 0, slots,
                                     rocprim::plus<int>(), stream));
    hipLaunchKernelGGL(k_cl_rowptr, dim3(capped_grid((size_t)N + 1, 256)), dim3(256), 0, stream, rowptr, rowptr_by_target, n, e, y, rp_o);
    hipLaunchKernelGGL(k_cl_fill, dim3(capped_grid(slots, 256)), dim3(256), 0, stream, rowptr, col, erow, rowptr_by_target, sources,
                       erow_by_target, e, code, y, rp_o, nbr_u);
    // the rows hold at most E entries in all (the exact count is on the device); the segments bound what is sorted
    int bits = 1;
    while (bits < 32 && (1ull << bits) < 2ull * (u64)N) ++bits;
    POPE_HIP(rocprim::segmented_radix_sort_keys(sort_tmp, sort_bytes, (const unsigned *)nbr_u, nbr, (unsigned)E, (unsigned)N,
                                                (const int *)rp_o, (const int *)rp_o + 1, 0, bits, stream));
    const size_t blocks = ((size_t)N + CL_WAVES - 1) / CL_WAVES;
    hipLaunchKernelGGL(k_cl_triangles, dim3((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(64 * CL_WAVES), 0, stream, rp_o,
                       nbr, n, (unsigned long long *)T);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}
