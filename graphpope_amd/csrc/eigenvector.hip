// Biased anchor selection on the device: eigenvector centrality for sampling_method='eigenvector_centrality'.
//
// Replaces the reference's utils.py:44-48  nx.eigenvector_centrality_numpy(to_networkx(data)): the eigenvector of M^T for
// the eigenvalue of largest real part, M the adjacency of the DiGraph (one edge per distinct (u, v) pair, self-loops kept),
// L2-normalised with a positive sum.  NetworkX gets it from ARPACK; here it is a shifted power iteration in float64:
//     x0 = 1 / sqrt(N);   ax = M^T x;   lambda = x . ax;   r = ||ax - lambda x||;   stop if r <= tol * lambda;
//     otherwise x <- (ax + x) / ||ax + x||       (the + x is a shift by the identity: it converges on periodic graphs too)
// Agreement with ARPACK is to a MEASURED tolerance, not bit for bit.  Nodes whose scores are mathematically
// equal (automorphic nodes) come out in a deterministic order here; NetworkX orders them by ARPACK's rounding noise.
//
// Three launches per iteration, the launch boundary being the only synchronisation (no grid barrier, no spin wait):
//   k_eig_spmv     ax = M^T x over the canonical CSR by target, and per-block partials of x . ax
//   k_eig_combine  lambda from the partials; per-block partials of ||ax - lambda x||^2 and ||ax + x||^2; ax <- ax + x
//   k_eig_finish   r and the norm from the partials; the stop test; x <- ax / norm unless it passed; the control block
// Every sum has a fixed order: a thread adds its elements in index order, a wave folds its lanes by a butterfly, a block adds
// its four waves in order, and EVERY block of the next launch adds the per-block partials by the same tree, so all blocks hold
// the same bits and take the same decision.  No floating-point atomics: two runs return the same bits, and because the grids
// depend on N alone, so do two devices.
// The loop is device-resident: a control block {iterations, lambda, r, done} lives in device memory; once `done` is set every
// kernel of the iterations queued behind returns without writing, so x is exactly the first vector that met the test.
#include "common.h"
#include "wave.h"

// Every multiply and add is rounded on its own (as in centrality.hip): the result does not depend on what the compiler
// would choose to fuse.
#pragma clang fp contract(off)

namespace pope {

constexpr int EIG_BLOCK = 256;            // threads per block: four waves
constexpr int EIG_MAX_BLOCKS = 1024;      // per-block partials of one reduction; the grid is a function of N alone
// Rows of at least this many entries are summed by a whole wave.  A row of 64 gives every lane of the wave an entry in its
// first load; below that a wave would leave lanes idle and still pay the six-step cross-lane fold (twelve ds_bpermute,
// about three L2-hit latencies), in which one thread walks several entries of a short row.  Chosen from those figures, not
// measured.
constexpr int EIG_WAVE_ROW = 64;
constexpr int EIG_ROW_UNROLL = 8;          // entries of a thread row whose loads are in flight together
constexpr int EIG_WAVE_UNROLL = 8;         // strides of a wave row whose gathers are in flight together

struct EigControl {                       // 32 bytes, device memory, zeroed by the caller before the first iteration
    long long iterations;                 // products ax = M^T x evaluated so far (the one that met the test included)
    double lambda;                        // x . ax of the last evaluated iteration
    double residual;                      // ||ax - lambda x||_2 of the last evaluated iteration
    int done;                             // 1 once residual <= tol * lambda
    int pad;
};
static_assert(sizeof(EigControl) == 32, "control block layout");

struct EigScratch {                       // offsets into the caller's scratch, bytes
    size_t ax, p_dot, p_res, p_nrm, lam, total;
    int blocks;
};

inline EigScratch eig_layout(int64_t N) {
    EigScratch s;
    s.blocks = (int)capped_grid((size_t)N, EIG_BLOCK, EIG_MAX_BLOCKS);
    size_t off = 0;
    s.ax = off;    off += align_up((size_t)N * sizeof(double), 256);
    s.p_dot = off; off += align_up((size_t)s.blocks * sizeof(double), 256);
    s.p_res = off; off += align_up((size_t)s.blocks * sizeof(double), 256);
    s.p_nrm = off; off += align_up((size_t)s.blocks * sizeof(double), 256);
    s.lam = off;   off += 256;
    s.total = off;
    return s;
}

// Sum over the block in a fixed order (lanes by butterfly, then the four waves in index order); every thread returns the
// same bits.  `lds` holds one double per wave and may be reused after the call returns.
__device__ __forceinline__ double block_sum(double v, double *lds) {
    v = wave_sum(v);
    __syncthreads();                                              // an earlier use of lds has been read
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int w = 1; w < EIG_BLOCK / 64; ++w) s = s + lds[w];
    return s;
}

// The per-block partials of the previous launch, added by the same tree in every block.
__device__ __forceinline__ double sum_partials(const double *__restrict__ p, int count, double *lds) {
    double s = 0.0;
    for (int k = threadIdx.x; k < count; k += EIG_BLOCK) s = s + p[k];
    return block_sum(s, lds);
}

// ax[i] = sum of x[j] over the distinct in-neighbours j of i;  p_dot[block] = sum over the block's rows of x[i] * ax[i].
// A block takes tiles of 256 rows: a thread walks its own row if it is short, rows of EIG_WAVE_ROW entries or more are
// queued in LDS and summed by the block's waves, one wave per row.  Whichever way a row is summed its order is fixed, and
// its owner thread adds x[i] * ax[i] to its partial in tile order.
__global__ __launch_bounds__(EIG_BLOCK) void k_eig_spmv(const int *__restrict__ rowptr_t, const int *__restrict__ src_t, int N,
                                                        const double *__restrict__ x, double *__restrict__ ax,
                                                        double *__restrict__ p_dot, const EigControl *__restrict__ ctl) {
    if (ctl->done) return;
    __shared__ int q_row[EIG_BLOCK];
    __shared__ double q_sum[EIG_BLOCK];
    __shared__ int q_count;
    __shared__ double lds[EIG_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles = (N + EIG_BLOCK - 1) / EIG_BLOCK;
    double dot = 0.0;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if (threadIdx.x == 0) q_count = 0;
        __syncthreads();
        const long long i = (long long)tile * EIG_BLOCK + threadIdx.x;   // 64-bit: the last tile may reach past 2^31
        double acc = 0.0;
        int slot = -1;
        if (i < N) {
            const int beg = rowptr_t[i], end = rowptr_t[i + 1];
            if (end - beg < EIG_WAVE_ROW) {
                // entries in order, EIG_ROW_UNROLL at a time: their column loads go out together, then their gathers, then
                // the additions in order -- the same sum as one entry at a time, without a dependent round trip per entry
                int prev = -1;
                for (int q = beg; q < end; q += EIG_ROW_UNROLL) {
                    int j[EIG_ROW_UNROLL];
                    double v[EIG_ROW_UNROLL];
#pragma unroll
                    for (int u = 0; u < EIG_ROW_UNROLL; ++u) j[u] = u < end - q ? src_t[q + u] : -1;
#pragma unroll
                    for (int u = 0; u < EIG_ROW_UNROLL; ++u) v[u] = j[u] >= 0 ? x[j[u]] : 0.0;
#pragma unroll
                    for (int u = 0; u < EIG_ROW_UNROLL; ++u) {
                        if (j[u] >= 0 && j[u] != prev) acc = acc + v[u];   // a repeated edge (adjacent, equal): one entry in the DiGraph
                        prev = j[u];
                    }
                }
                ax[i] = acc;
            } else {
                slot = atomicAdd(&q_count, 1);                    // integer, LDS: the order of the queue changes no sum
                q_row[slot] = (int)i;
            }
        }
        __syncthreads();
        const int queued = q_count;
        for (int k = wave; k < queued; k += EIG_BLOCK / 64) {
            const int row = q_row[k];
            const int beg = rowptr_t[row], end = rowptr_t[row + 1];
            double part = 0.0;
            // lane l adds entries l, l + 64, ... in that order.  The loads of EIG_WAVE_UNROLL strides are issued together and
            // the additions follow in order: the same sum, with that many gathers in flight instead of one (a row of 5 600
            // entries is 88 strides, each a dependent L2 or HBM round trip if taken one at a time).
            long long q = (long long)beg + lane;
            for (; q + (EIG_WAVE_UNROLL - 1) * 64 < end; q += EIG_WAVE_UNROLL * 64) {
                int j[EIG_WAVE_UNROLL];
                bool repeated[EIG_WAVE_UNROLL];
                double v[EIG_WAVE_UNROLL];
#pragma unroll
                for (int u = 0; u < EIG_WAVE_UNROLL; ++u) {
                    const long long qu = q + u * 64;
                    j[u] = src_t[qu];
                    repeated[u] = qu > beg && j[u] == src_t[qu - 1];   // a repeated edge: one entry in the DiGraph
                }
#pragma unroll
                for (int u = 0; u < EIG_WAVE_UNROLL; ++u) v[u] = x[j[u]];
#pragma unroll
                for (int u = 0; u < EIG_WAVE_UNROLL; ++u) part = part + (repeated[u] ? 0.0 : v[u]);
            }
            for (; q < end; q += 64) {
                const int j = src_t[q];
                const bool repeated = q > beg && j == src_t[q - 1];
                const double v = x[j];
                part = part + (repeated ? 0.0 : v);
            }
            part = wave_sum(part);
            if (lane == 0) {
                ax[row] = part;
                q_sum[k] = part;
            }
        }
        __syncthreads();
        if (slot >= 0) acc = q_sum[slot];
        if (i < N) {
            const double prod = x[i] * acc;
            dot = dot + prod;
        }
    }
    dot = block_sum(dot, lds);
    if (threadIdx.x == 0) p_dot[blockIdx.x] = dot;
}

// lambda = sum of p_dot;  d = ax - lambda x, y = ax + x;  p_res[block] = sum d^2, p_nrm[block] = sum y^2;  ax <- y.
__global__ __launch_bounds__(EIG_BLOCK) void k_eig_combine(int N, const double *__restrict__ x, double *__restrict__ ax,
                                                           const double *__restrict__ p_dot, double *__restrict__ p_res,
                                                           double *__restrict__ p_nrm, double *__restrict__ lam_out,
                                                           const EigControl *__restrict__ ctl) {
    if (ctl->done) return;
    __shared__ double lds[EIG_BLOCK / 64];
    const double lam = sum_partials(p_dot, gridDim.x, lds);
    double res = 0.0, nrm = 0.0;
    for (long long i = (long long)blockIdx.x * EIG_BLOCK + threadIdx.x; i < N; i += (long long)gridDim.x * EIG_BLOCK) {
        const double a = ax[i], xi = x[i];
        const double lx = lam * xi;
        const double d = a - lx;
        const double dd = d * d;
        res = res + dd;
        const double y = a + xi;
        const double yy = y * y;
        nrm = nrm + yy;
        ax[i] = y;
    }
    res = block_sum(res, lds);
    nrm = block_sum(nrm, lds);
    if (threadIdx.x == 0) {
        p_res[blockIdx.x] = res;
        p_nrm[blockIdx.x] = nrm;
        if (blockIdx.x == 0) *lam_out = lam;
    }
}

// r = sqrt(sum p_res), norm = sqrt(sum p_nrm).  Every block holds the same r, lambda and norm and so takes the same branch:
// if r <= tol * lambda nobody writes x and block 0 sets `done`; otherwise x <- y / norm.
// This is the one launch in which `done` is written while other blocks may still be starting, so a block reads it ONCE
// (thread 0, handed to the others through LDS behind a barrier): the block leaves whole or stays whole, never with some of its
// waves gone ahead of the barriers below.  A block that reads 1 there returns: block 0 set it in this launch because the test
// passed, and then this block would not have written x either.  A block that reads 0 computes the same r as block 0.
__global__ __launch_bounds__(EIG_BLOCK) void k_eig_finish(int N, double *__restrict__ x, const double *__restrict__ y,
                                                          const double *__restrict__ p_res, const double *__restrict__ p_nrm,
                                                          const double *__restrict__ lam_in, double tol, EigControl *__restrict__ ctl) {
    __shared__ int done_before;
    __shared__ double lds[EIG_BLOCK / 64];
    if (threadIdx.x == 0) done_before = ctl->done;
    __syncthreads();
    if (done_before) return;
    const double r = sqrt(sum_partials(p_res, gridDim.x, lds));
    const double norm = sqrt(sum_partials(p_nrm, gridDim.x, lds));
    const double lam = *lam_in;
    const double bound = tol * lam;
    const bool converged = r <= bound;
    if (!converged)
        for (long long i = (long long)blockIdx.x * EIG_BLOCK + threadIdx.x; i < N; i += (long long)gridDim.x * EIG_BLOCK) x[i] = y[i] / norm;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->iterations = ctl->iterations + 1;
        ctl->lambda = lam;
        ctl->residual = r;
        if (converged) ctl->done = 1;
    }
}

}  // namespace pope

using namespace pope;

extern "C" size_t pope_eigenvector_scratch_bytes(int64_t N) {
    clear_error();
    if (N <= 0 || N >= INT32_MAX) return 0;
    return eig_layout(N).total;
}

extern "C" int pope_eigenvector_iterate(const int32_t *rowptr_by_target, const int32_t *sources, int64_t N, double *x, void *scratch,
                                        size_t scratch_bytes, int32_t iterations, double tol, void *control, void *stream_) {
    clear_error();
    POPE_REQUIRE(rowptr_by_target && sources && x && scratch && control, "pope_eigenvector_iterate: null pointer");
    POPE_REQUIRE(N > 0 && N < INT32_MAX, "pope_eigenvector_iterate: N = %lld outside (0, 2^31 - 1)", (long long)N);
    POPE_REQUIRE(iterations > 0, "pope_eigenvector_iterate: iterations = %d, expected at least 1", (int)iterations);
    POPE_REQUIRE(tol > 0.0, "pope_eigenvector_iterate: tol = %g, expected a positive number", tol);
    const EigScratch s = eig_layout(N);
    if (scratch_bytes < s.total) {
        set_error("pope_eigenvector_iterate: scratch of %zu bytes, pope_eigenvector_scratch_bytes(N) = %zu", scratch_bytes, s.total);
        return POPE_ERR_WORKSPACE;
    }
    char *base = (char *)scratch;
    double *ax = (double *)(base + s.ax), *p_dot = (double *)(base + s.p_dot), *p_res = (double *)(base + s.p_res);
    double *p_nrm = (double *)(base + s.p_nrm), *lam = (double *)(base + s.lam);
    EigControl *ctl = (EigControl *)control;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid(s.blocks), block(EIG_BLOCK);
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(k_eig_spmv, grid, block, 0, stream, rowptr_by_target, sources, (int)N, x, ax, p_dot, ctl);
        hipLaunchKernelGGL(k_eig_combine, grid, block, 0, stream, (int)N, x, ax, p_dot, p_res, p_nrm, lam, ctl);
        hipLaunchKernelGGL(k_eig_finish, grid, block, 0, stream, (int)N, x, ax, p_res, p_nrm, lam, tol, ctl);
    }
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}
