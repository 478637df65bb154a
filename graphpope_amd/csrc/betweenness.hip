// Biased anchor selection on the device: betweenness scores for sampling_method='betweenness_centrality'.
//
// Replaces /root/reference/utils.py:32-36  nx.betweenness_centrality(to_networkx(data)).  The anchors are the last K keys
// of an ascending stable sort of float64 scores, tied nodes are common and their ROUNDING decides the order, so the scores
// are reproduced BIT FOR BIT: every float64 addition NetworkX 3.4.2 performs is performed here, in its order.
//   * G[v] of the DiGraph iterates v's successors in the order each distinct (v, w) first appears in edge_index: the CSR by
//     source arrives in that "insertion order", one slot per distinct pair (engine.insertion_csr).
//   * per source s (_single_source_shortest_path_basic): a FIFO queue; v is dequeued; for w in G[v]: an unseen w is enqueued
//     with D[w] = D[v] + 1; if D[w] == D[v] + 1: sigma[w] += sigma[v].
//   * _accumulate_basic: the queue is walked from its end; coeff = (1 + delta[w]) / sigma[w]; every predecessor v of w gets
//     delta[v] += sigma[v] * coeff -- a rounded product, then a rounded sum; if w != s: betweenness[w] += delta[w].
//   * sources run in node order, so betweenness[w] is the left-to-right sum of delta_s[w] over s ascending (k_bc_sum).
//   * _rescale is one multiplication per node, done by the host binding.
// Inside one step the lanes of a wave work in parallel without changing a sum: the successors of one v are distinct nodes
// and so are the predecessors of one w, and each of them receives exactly one addition in that step.  The queue itself
// stays serial per source; the parallelism is across sources: one wave64 per source (k_bc_replay), N independent sources.
//
// Workspace of a batch of B sources: one 32-byte record {sigma, delta, dist} per (source, node), so that a touched
// neighbour costs one sector, the queue int32 [B, N] (after the forward pass it is NetworkX's stack S), its length [B].
#include "common.h"

// Every multiply and add is rounded on its own (see centrality.hip): delta[v] += sigma[v] * coeff must not become an fma.
#pragma clang fp contract(off)

namespace pope {

constexpr int BC_WAVES = 4;          // waves (sources in flight) per 256-thread block
constexpr int BC_BLOCKS_PER_CU = 8;  // 32 waves per CU: the per-source chain is latency-bound, occupancy hides it

struct alignas(32) BcNode {
    double sigma;                    // shortest paths from the source
    double delta;                    // dependency of the source on this node
    int dist;                        // -1 = not reached
    int pad[3];
};
static_assert(sizeof(BcNode) == 32, "one record = one 32-byte sector");

// The lanes of one wave hand values to each other through global memory (lane i stores sigma[w], lane j loads it some
// steps later).  A wave's vector memory operations are performed in order, so no instruction is needed; this keeps the
// compiler from moving a step's loads above the previous step's stores.
__device__ __forceinline__ void wave_mem_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Row bounds of node v, clamped to the slots the caller passed: a malformed CSR cannot send a lane out of bounds.
__device__ __forceinline__ void row_bounds(const int *__restrict__ rp, int v, int N, int nnz, int &beg, int &end) {
    const bool ok = (unsigned)v < (unsigned)N;
    beg = ok ? max(rp[v], 0) : 0;
    end = ok ? min(rp[v + 1], nnz) : 0;
}

__global__ __launch_bounds__(64 * BC_WAVES) void k_bc_replay(const int *__restrict__ rp_s, const int *__restrict__ col_s, int nnz_s,
                                                             const int *__restrict__ rp_t, const int *__restrict__ col_t, int nnz_t, int N,
                                                             int first, int ns, BcNode *rec_all, int *queue_all, int *qlen) {
    const int lane = threadIdx.x & 63;
    const u64 below = (1ull << lane) - 1ull;
    for (int b = blockIdx.x * BC_WAVES + (threadIdx.x >> 6); b < ns; b += gridDim.x * BC_WAVES) {
        const int s = first + b;
        BcNode *rec = rec_all + (size_t)b * (size_t)N;
        int *q = queue_all + (size_t)b * (size_t)N;
        BcNode blank;
        blank.sigma = 0.0;
        blank.delta = 0.0;
        blank.dist = -1;
        blank.pad[0] = blank.pad[1] = blank.pad[2] = 0;
        for (int t = lane; t < N; t += 64) rec[t] = blank;
        wave_mem_sync();
        if (lane == 0) {
            rec[s].sigma = 1.0;
            rec[s].dist = 0;
            q[0] = s;
        }
        wave_mem_sync();

        // forward: NetworkX's BFS, the queue in NetworkX's order
        int head = 0, tail = 1;
        int vv = s, beg, end;
        row_bounds(rp_s, s, N, nnz_s, beg, end);
        while (true) {
            ++head;
            // the next queue entry, if it is known already, and its row bounds: loaded underneath this row's work
            const bool ahead = head < tail;
            int nvv = 0, nbeg = 0, nend = 0;
            if (ahead) {
                nvv = q[head];
                row_bounds(rp_s, __builtin_amdgcn_readfirstlane(nvv), N, nnz_s, nbeg, nend);
            }
            const double sv = rec[vv].sigma;
            const int dnext = rec[vv].dist + 1;
            for (int lo = beg; lo < end; lo += 64) {
                const int idx = lo + lane;
                bool valid = idx < end;
                const int w = valid ? col_s[idx] : 0;
                valid = valid && (unsigned)w < (unsigned)N;
                const int dw = valid ? rec[w].dist : 0;
                const bool unseen = valid && dw < 0;
                const u64 mask = __ballot(unseen);
                const int pos = tail + __popcll(mask & below);    // lane order = adjacency order
                if (unseen && pos < N) {
                    q[pos] = w;
                    rec[w].dist = dnext;
                }
                if (valid && (unseen || dw == dnext)) rec[w].sigma = rec[w].sigma + sv;
                tail = min(tail + (int)__popcll(mask), N);
                wave_mem_sync();
            }
            if (head >= tail) break;
            if (!ahead) {
                nvv = q[head];
                row_bounds(rp_s, __builtin_amdgcn_readfirstlane(nvv), N, nnz_s, nbeg, nend);
            }
            if ((unsigned)nvv >= (unsigned)N) break;              // cannot happen: every entry below tail was written above
            vv = nvv;
            beg = nbeg;
            end = nend;
        }
        if (lane == 0) qlen[b] = tail;

        // backward: the queue from its end; q[0] = s has no predecessor on a shortest path
        if (tail > 1) {
            int ww = q[tail - 1];
            row_bounds(rp_t, __builtin_amdgcn_readfirstlane(ww), N, nnz_t, beg, end);
            for (int i = tail - 1; i >= 1; --i) {
                int nww = 0, nbeg = 0, nend = 0;
                if (i > 1) {
                    nww = q[i - 1];
                    row_bounds(rp_t, __builtin_amdgcn_readfirstlane(nww), N, nnz_t, nbeg, nend);
                }
                if ((unsigned)ww >= (unsigned)N) break;
                const BcNode rw = rec[ww];
                const double one_plus = 1.0 + rw.delta;
                const double coeff = one_plus / rw.sigma;
                const int dprev = rw.dist - 1;
                for (int lo = beg; lo < end; lo += 64) {
                    const int idx = lo + lane;
                    bool valid = idx < end;
                    const int p = valid ? col_t[idx] : 0;
                    valid = valid && (unsigned)p < (unsigned)N;
                    if (valid) {
                        const BcNode pr = rec[p];
                        if (pr.dist == dprev) {
                            const double prod = pr.sigma * coeff;
                            rec[p].delta = pr.delta + prod;
                        }
                    }
                }
                wave_mem_sync();
                ww = nww;
                beg = nbeg;
                end = nend;
            }
        }
    }
}

// bc[w] += delta_b[w] for the batch's sources b ascending: with the batches run in source order this is NetworkX's
// left-to-right sum.  The source's own delta is not added; nodes a source did not reach hold +0.0.
__global__ __launch_bounds__(256) void k_bc_sum(const BcNode *__restrict__ rec, int N, int first, int ns, double *__restrict__ bc) {
    for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < N; w += gridDim.x * blockDim.x) {
        double acc = bc[w];
        const BcNode *r = rec + w;
        for (int b = 0; b < ns; ++b, r += N) {
            const double d = r->delta;
            if (first + b != w) acc = acc + d;
        }
        bc[w] = acc;
    }
}

// The per-source rows as dense arrays [ns, N] (diagnostics and tests).
__global__ __launch_bounds__(256) void k_bc_rows(const BcNode *__restrict__ rec, size_t total, double *__restrict__ sigma,
                                                 double *__restrict__ delta, int *__restrict__ dist) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const BcNode r = rec[i];
        if (sigma) sigma[i] = r.sigma;
        if (delta) delta[i] = r.delta;
        if (dist) dist[i] = r.dist;
    }
}

}  // namespace pope

using namespace pope;

namespace {

constexpr int64_t BC_MAX_CELLS = 1ll << 40;           // (source, node) pairs of one batch: 32 TiB of records, beyond any device

struct BcScratch {
    size_t rec, queue, qlen, total;
};

bool bc_sizes_ok(int64_t N, int64_t batch) { return N > 0 && N < INT32_MAX && batch > 0 && batch <= N && batch <= BC_MAX_CELLS / N; }

// records [batch, N] 32 B | queue [batch, N] int32 | queue length [batch] int32
BcScratch bc_layout(int64_t N, int64_t batch) {
    BcScratch L;
    const size_t cells = (size_t)N * (size_t)batch;
    size_t o = 0;
    L.rec = o;   o += align_up(cells * sizeof(BcNode), 256);
    L.queue = o; o += align_up(cells * sizeof(int), 256);
    L.qlen = o;  o += align_up((size_t)batch * sizeof(int), 256);
    L.total = o;
    return L;
}

}  // namespace

extern "C" size_t pope_betweenness_scratch_bytes(int64_t N, int64_t batch) {
    return bc_sizes_ok(N, batch) ? bc_layout(N, batch).total : 0;
}

extern "C" int pope_betweenness_batch(const int32_t *rowptr, const int32_t *col, int64_t E_by_source, const int32_t *rowptr_by_target,
                                      const int32_t *sources, int64_t E_by_target, int64_t N, int64_t first_source,
                                      int64_t num_sources, double *bc, double *sigma_out, double *delta_out, int32_t *dist_out,
                                      int32_t *queue_len_out, void *scratch, size_t scratch_bytes, void *stream_) {
    clear_error();
    POPE_REQUIRE(N > 0 && N < INT32_MAX, "pope_betweenness_batch: need 0 < N < 2^31 (N=%lld)", (long long)N);
    POPE_REQUIRE(E_by_source >= 0 && E_by_target >= 0 && E_by_source < INT32_MAX && E_by_target < INT32_MAX,
                 "pope_betweenness_batch: the CSR slots (%lld by source, %lld by target) do not fit int32 offsets",
                 (long long)E_by_source, (long long)E_by_target);
    POPE_REQUIRE(first_source >= 0 && num_sources > 0 && first_source <= N - num_sources,
                 "pope_betweenness_batch: sources [%lld, %lld + %lld) are not nodes of a graph of %lld", (long long)first_source,
                 (long long)first_source, (long long)num_sources, (long long)N);
    POPE_REQUIRE(num_sources <= BC_MAX_CELLS / N, "pope_betweenness_batch: a batch of %lld sources x %lld nodes is too large",
                 (long long)num_sources, (long long)N);
    POPE_REQUIRE(rowptr && rowptr_by_target && bc && scratch && (col || E_by_source == 0) && (sources || E_by_target == 0),
                 "pope_betweenness_batch: null pointer");
    const BcScratch L = bc_layout(N, num_sources);
    if (scratch_bytes < L.total) {
        set_error("pope_betweenness_batch: scratch %zu < %zu bytes", scratch_bytes, L.total);
        return POPE_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const int n = (int)N, ns = (int)num_sources, first = (int)first_source;
    char *base = (char *)scratch;
    BcNode *rec = (BcNode *)(base + L.rec);
    int *queue = (int *)(base + L.queue), *qlen = (int *)(base + L.qlen);

    int dev = 0, cus = 0;
    POPE_HIP(hipGetDevice(&dev));
    POPE_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const unsigned resident = (unsigned)(cus > 0 ? cus : 256) * BC_BLOCKS_PER_CU;
    const unsigned blocks = (unsigned)((ns + BC_WAVES - 1) / BC_WAVES);
    hipLaunchKernelGGL(k_bc_replay, dim3(blocks < resident ? blocks : resident), dim3(64 * BC_WAVES), 0, stream, rowptr, col,
                       (int)E_by_source, rowptr_by_target, sources, (int)E_by_target, n, first, ns, rec, queue, qlen);
    hipLaunchKernelGGL(k_bc_sum, dim3(capped_grid((size_t)N, 256)), dim3(256), 0, stream, rec, n, first, ns, bc);
    if (sigma_out || delta_out || dist_out) {
        const size_t total = (size_t)N * (size_t)ns;
        hipLaunchKernelGGL(k_bc_rows, dim3(capped_grid(total, 256)), dim3(256), 0, stream, rec, total, sigma_out, delta_out, dist_out);
    }
    if (queue_len_out) POPE_HIP(hipMemcpyAsync(queue_len_out, qlen, (size_t)ns * sizeof(int), hipMemcpyDeviceToDevice, stream));
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}
