// node2vec on the GPU: uniform random walks, the skip-gram loss with its gradient, and SparseAdam.
//
// Replaces what /root/reference/generate_node2vec_embedding.py:23-25 builds out of PyG: Node2Vec(p = 1, q = 1, sparse = True), i.e.
// torch_cluster.random_walk for pos_sample, torch.randint for neg_sample, Node2Vec.loss and torch.optim.SparseAdam.
//
//   k_n2v_walks        one thread per row.  Positive row i: L uniform steps from starts[i] over the forward CSR (a node without
//                      out-neighbours stays where it is: torch_cluster's rule).  Negative row i: starts[i], then L nodes uniform on [0, N).
//                      The draw at (row, step) is a counter hash of (seed, first_row + i, step, positive-or-negative): a row depends on
//                      nothing else -- not on B, not on the launch geometry, not on the other rows of the call.
//   k_n2v_walks_biased one WAVE per positive row of a second-order (p, q) walk: step 0 as above; then 16 rejection tries taken side
//                      by side, one per lane (a candidate slot of the row, weight 1/p back to the previous node t, 1 to an
//                      out-neighbour of t -- a binary search in t's ascending row -- and 1/q elsewhere, accepted with probability
//                      w / w_max; the first accepted try counts) and, with none accepted, an exact inverse-CDF pass over the
//                      row by the whole wave.  p = q = 1 accepts try 0: k_n2v_walks' rows.
//   k_n2v_windows      [R, len] rows -> PyG's window matrix [(len + 1 - C) * R, C], window j of row r at j * R + r.
//   k_n2v_loss_grad    one wave per 8 consecutive rows, a row at a time.  The row's len embedding rows go to LDS once; the (len + 1 - C)(C - 1) products
//                      <emb[w_j], emb[w_{j+k}]> are taken there, one product per lane, in float64; every term is evaluated literally as
//                      -log(sigmoid(out) + 1e-15) or -log(1 - sigmoid(out) + 1e-15), in float64 too, so a saturated product gives what the
//                      formula gives and not what a log-sigmoid identity would.  The gradient of every walk POSITION is then summed in
//                      registers over all windows it takes part in (as start and as context): len rows per walk instead of
//                      (len + 1 - C) * C (21 against 120 at the reference's shape).  The rows of the first 16 distinct nodes the wave meets
//                      are summed in LDS over its 8 walks and leave as one row of atomic adds each at the end; the others leave at once.  Lane l owns the
//                      columns l, l + 64, ...: each atomic wave-instruction covers 256 contiguous bytes, the shape that runs at the
//                      chip's full float-atomic rate.  The loss leaves the wave as one float64 atomic add per wave.
//   k_n2v_sparse_adam  one launch over the N rows: a block reads 64 flags at once and its 4 waves update only the flagged rows
//                      (torch.optim.SparseAdam: the moments of the other rows do not decay), clearing their gradient rows and flags on
//                      the way; every operation of the update is one float32 operation rounded once (no FMA contraction).
//
// Deterministic mode (sage_set_deterministic(1): graphpope_amd.node2vec calls the next two in place of pope_n2v_loss_grad):
//   k_n2v_position_grads  k_n2v_loss_grad up to the register sums: one wave per row, no merge table, no atomics.  Position i of row r
//                      STORES its gradient row to contrib[r * len + i] and its node to ids[r * len + i]; the row's loss goes to row_loss[r].
//   k_n2v_det_clear, k_n2v_det_index, k_n2v_det_scan   the inverted index of ids in the scratch buffer: det_index.h's format and bodies
//                      (the ones sage.hip's k_det_* wrap too); k_n2v_det_index is this file's producer, one thread per entry ...
//   k_n2v_det_rank     ... lists longer than a wave brought into ascending order: one thread per slot ranks its entry against its list ...
//   k_n2v_sum_det      ... and one wave per node that adds the list's contrib rows in ascending entry order (a list of up to 64 entries
//                      is sorted in registers, bitonic), in float64, rounding once into grad.
//   k_n2v_loss_sum     one block: the float64 sum of row_loss in an order that depends on R alone, one plain add into loss_acc.
//
// NOT reproducible bit for bit: k_n2v_loss_grad's gradient (float atomic adds land in arrival order, so its last bits differ between two
// runs) and the last bits of its float64 loss.  Reproducible bit for bit: walks, negatives, windows, SparseAdam, and the deterministic pair.
#include "common.h"
#include "det_index.h"

namespace pope {

__host__ __device__ __forceinline__ u64 n2v_mix64(u64 z) {                     // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// 32 uniform bits for (seed, row, step, kind): keyed on the row AND on the step, so the steps of one row are independent draws.
__host__ __device__ __forceinline__ unsigned n2v_draw(u64 seed, u64 row, unsigned step, unsigned kind) {
    const u64 row_key = n2v_mix64(seed + 0x9E3779B97F4A7C15ull * (2ull * row + kind + 1ull));
    return (unsigned)(n2v_mix64(row_key ^ (0xD1B54A32D192ED03ull * (u64)(step + 1u))) >> 32);
}

// uniform on [0, n), n < 2^31: the high word of draw * n (bias below n / 2^32)
__host__ __device__ __forceinline__ long long n2v_below(unsigned draw, long long n) { return (long long)(((u64)draw * (u64)n) >> 32); }

__global__ __launch_bounds__(256) void k_n2v_walks(const int *__restrict__ rowptr, const int *__restrict__ col, long long N,
                                                   const long long *__restrict__ starts, long long B, long long B_neg, int L, u64 seed,
                                                   long long first_row, long long *__restrict__ pos, long long *__restrict__ neg) {
    const long long total = B + B_neg;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const bool negative = t >= B;
        const long long i = negative ? t - B : t;
        const long long start = starts[i];
        long long *__restrict__ out = (negative ? neg : pos) + i * (long long)(L + 1);
        out[0] = start;
        const u64 row = (u64)(first_row + i);
        if (negative) {
            for (int s = 0; s < L; ++s) out[s + 1] = n2v_below(n2v_draw(seed, row, (unsigned)s, 1u), N);
        } else {
            long long cur = start;
            const bool valid = start >= 0 && start < N;              // a start outside the graph reads nothing and stays put
            for (int s = 0; s < L; ++s) {
                if (valid) {
                    const int lo = rowptr[cur], deg = rowptr[cur + 1] - lo;
                    if (deg > 0) cur = col[lo + (int)n2v_below(n2v_draw(seed, row, (unsigned)s, 0u), deg)];
                }
                out[s + 1] = cur;
            }
        }
    }
}

// ---- second-order (p, q) walks ---------------------------------------------------------------------------------------------------
// The draws of step s of a row: step_key = mix64(seed + G (2 row + 1)) ^ (D (s + 1)), then try j draws its candidate from
// mix64(step_key + G (2 j)) and its acceptance from mix64(step_key + G (2 j + 1)), the high words.  (s, j = 0, candidate) is
// n2v_draw(seed, row, s, 0): the first-order kernel's draw.
constexpr int N2V_TRIES = 16;

__host__ __device__ __forceinline__ unsigned n2v_draw2(u64 step_key, unsigned j, unsigned which) {
    return (unsigned)(n2v_mix64(step_key + 0x9E3779B97F4A7C15ull * (u64)(2u * j + which)) >> 32);
}

constexpr int N2V_PER_LANE = 4;                                   // slots a lane classifies per round of the exact pass
constexpr int N2V_ROUND = 64 * N2V_PER_LANE;

// x[u] among col[lo .. lo + deg), an ASCENDING row, for K values at once: lower bounds whose trip count depends on deg
// alone (at most 31 halvings, deg < 2^31), so the searches advance together and their loads overlap.  The bound lies at base or
// base + 1 when the loop ends.  Every read lies inside the row whatever its order; on an unsorted row the answer may be wrong.
template <int K>
__device__ __forceinline__ void n2v_row_has(const int *__restrict__ col, int lo, int deg, const int (&x)[K], bool (&has)[K]) {
    int base[K];
#pragma unroll
    for (int u = 0; u < K; ++u) {
        base[u] = lo;
        has[u] = false;
    }
    if (deg <= 0) return;
    for (int len = deg; len > 1;) {
        const int half = len >> 1;
#pragma unroll
        for (int u = 0; u < K; ++u) base[u] += col[base[u] + half - 1] < x[u] ? half : 0;   // base + len never grows
        len -= half;
    }
#pragma unroll
    for (int u = 0; u < K; ++u) {
        const int at = col[base[u]];
        has[u] = at == x[u] || (at < x[u] && base[u] + 1 < lo + deg && col[base[u] + 1] == x[u]);
    }
}

// The weights of the up to N2V_ROUND slots col[lo + c0 ..) of v's row, slot c0 + 64 u + b in wt[u] of lane b: 1/p if the slot is t
// itself, 1 if it is another out-neighbour of t, else 1/q (0 past the row's end, never added).
__device__ __forceinline__ void n2v_round_weights(const int *__restrict__ col, int lo, int deg, long long c0, int lane, int t, int tlo, int tdeg,
                                                  double inv_p, double inv_q, double (&wt)[N2V_PER_LANE]) {
    int x[N2V_PER_LANE];
    bool in[N2V_PER_LANE], has[N2V_PER_LANE];
#pragma unroll
    for (int u = 0; u < N2V_PER_LANE; ++u) {
        const long long k = c0 + 64 * u + lane;
        in[u] = k < deg;
        x[u] = in[u] ? col[lo + (int)k] : 0;
    }
    n2v_row_has<N2V_PER_LANE>(col, tlo, tdeg, x, has);
#pragma unroll
    for (int u = 0; u < N2V_PER_LANE; ++u) wt[u] = !in[u] ? 0.0 : x[u] == t ? inv_p : has[u] ? 1.0 : inv_q;
}

// One WAVE per walk; every value below but `lane` is wave-uniform, and so is every branch.  Step 0 is the first-order step.  Step
// s >= 1: lane j < N2V_TRIES evaluates rejection try j (candidate uniform over the row's slots, accepted with probability
// w / w_max) -- the tries are independent draws, so they are taken side by side and the FIRST accepted one counts, as if they had
// been made in turn.  No try accepted: the exact inverse-CDF pass over the row's weights, N2V_ROUND slots weighed per round, one
// search per slot and lane, and the weights added in slot order, in double, the same sequence of additions in every lane.  The
// mixture is the node2vec distribution itself.  Every loop is bounded by a constant or by a row's degree, whatever p, q and the graph.
// A lane per walk, as k_n2v_walks has it, left the launch waiting for the few lanes that stand on a hub: 70 ms at 1 280 walks on
// the Flickr-shaped graph with (p, q) = (0.25, 4), and 14 ms with the wave serving its lanes' exact passes in turn; this form: 1.8 ms
// (DESIGN 7l-2).  What is left is a hub's row: its 5 622 weights are added one after the other, for W and again for the prefix sums.
__global__ __launch_bounds__(256) void k_n2v_walks_biased(const int *__restrict__ rowptr, const int *__restrict__ col, long long N,
                                                          const long long *__restrict__ starts, long long B, int L, u64 seed,
                                                          long long first_row, double inv_p, double inv_q, double w_max,
                                                          long long *__restrict__ pos) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long i = wave; i < B; i += waves) {
        const long long start = starts[i];
        long long *__restrict__ out = pos + i * (long long)(L + 1);
        if (lane == 0) out[0] = start;
        const u64 row_key = n2v_mix64(seed + 0x9E3779B97F4A7C15ull * (2ull * (u64)(first_row + i) + 1ull));
        const bool valid = start >= 0 && start < N;                  // a start outside the graph reads nothing and stays put
        int cur = valid ? (int)start : 0;
        int t = 0, tlo = 0, tdeg = 0;                                // the previous node and its row: set by every move
        for (int s = 0; s < L; ++s) {
            int lo = 0, deg = 0;
            if (valid) {
                lo = rowptr[cur];
                deg = rowptr[cur + 1] - lo;
            }
            if (deg > 0) {                                           // out-degree 0: the walker stays and t does not change
                const u64 key = row_key ^ (0xD1B54A32D192ED03ull * (u64)(s + 1));
                int next;
                if (s == 0) {                                        // (s >= 1 with deg > 0: step s - 1 moved, so t is set)
                    next = col[lo + (int)n2v_below(n2v_draw2(key, 0u, 0u), deg)];
                } else {
                    const bool trying = lane < N2V_TRIES;
                    int x[1] = {0};
                    bool has[1];
                    if (trying) x[0] = col[lo + (int)n2v_below(n2v_draw2(key, (unsigned)lane, 0u), deg)];
                    n2v_row_has<1>(col, tlo, tdeg, x, has);          // (the lanes without a try search for node 0: reads inside t's row)
                    const double w = x[0] == t ? inv_p : has[0] ? 1.0 : inv_q;
                    const u64 accepted = __ballot(trying && (double)n2v_draw2(key, (unsigned)lane, 1u) * w_max < w * 4294967296.0);
                    if (accepted) {
                        next = __shfl(x[0], __ffsll((long long)accepted) - 1);
                    } else {                                         // the exact pass: W in slot order, then the first prefix sum above the target
                        double wt0[N2V_PER_LANE];                    // round 0's weights: all there is for a row of up to N2V_ROUND slots
                        double W = 0.0;
                        for (long long c0 = 0; c0 < deg; c0 += N2V_ROUND) {
                            double wt[N2V_PER_LANE];
                            n2v_round_weights(col, lo, deg, c0, lane, t, tlo, tdeg, inv_p, inv_q, wt);
#pragma unroll
                            for (int u = 0; u < N2V_PER_LANE; ++u) {
                                if (c0 == 0) wt0[u] = wt[u];
                                const int cnt = (int)max(0ll, min(64ll, (long long)deg - c0 - 64 * u));
                                for (int b = 0; b < cnt; ++b) W += wave_read_lane(wt[u], b);
                            }
                        }
                        const double target = (double)n2v_draw2(key, (unsigned)N2V_TRIES, 0u) * (1.0 / 4294967296.0) * W;
                        double run = 0.0;
                        long long slot = -1;
                        for (long long c0 = 0; c0 < deg && slot < 0; c0 += N2V_ROUND) {
                            double wt[N2V_PER_LANE];
                            if (c0 == 0) {
#pragma unroll
                                for (int u = 0; u < N2V_PER_LANE; ++u) wt[u] = wt0[u];
                            } else {
                                n2v_round_weights(col, lo, deg, c0, lane, t, tlo, tdeg, inv_p, inv_q, wt);
                            }
#pragma unroll
                            for (int u = 0; u < N2V_PER_LANE; ++u) {
                                const int cnt = (int)max(0ll, min(64ll, (long long)deg - c0 - 64 * u));
                                for (int b = 0; b < cnt && slot < 0; ++b) {
                                    run += wave_read_lane(wt[u], b);
                                    if (run > target) slot = c0 + 64 * u + b;
                                }
                            }
                        }
                        next = col[lo + (int)(slot < 0 ? deg - 1 : slot)];
                    }
                }
                t = cur;
                tlo = lo;
                tdeg = deg;
                cur = next;
            }
            if (lane == 0) out[s + 1] = valid ? (long long)cur : start;
        }
    }
}

__global__ __launch_bounds__(256) void k_n2v_windows(const long long *__restrict__ rows, long long R, int len, int C,
                                                     long long *__restrict__ out) {
    const int W = len + 1 - C;
    const long long total = (long long)W * R * C;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(t % C);
        const long long m = t / C, r = m % R;
        const int j = (int)(m / R);
        out[t] = rows[r * len + j + c];
    }
}

// A wave takes N2V_ROWS_PER_WAVE consecutive rows and keeps the gradient rows of the first N2V_SLOTS distinct nodes it meets in LDS: what
// its rows add to the same node -- a start shared by its walks, a hub, the two nodes of a 2-cycle -- is summed there in float32 and leaves
// as ONE atomic row.  Besides the bytes saved, this keeps the chain of float atomic adds on one address short: 1 600 adds onto the two
// rows of a 2-node graph left a relative error of 1.1e-5 (torch float32: 3.3e-7) before the rows were merged.
constexpr int N2V_ROWS_PER_WAVE = 8;
constexpr int N2V_SLOTS = 16;

// LDS of one wave: the row's embedding rows at a stride of D + 1 floats (lanes that read different rows at the same column hit different
// banks), the coefficient of every (window, context slot) pair, the node ids, and the N2V_SLOTS merged gradient rows with their keys.
__host__ __device__ inline size_t n2v_lds_bytes(int len, int C, int D) {
    return ((size_t)len * (size_t)(D + 1) + (size_t)(len + 1 - C) * (size_t)(C - 1) + (size_t)N2V_SLOTS * (size_t)D) * sizeof(float) +
           (size_t)(len + N2V_SLOTS) * sizeof(int);
}

// NK = ceil(D / 64): lane l owns columns l + 64 k, k < NK (those below D).
template <int NK>
__global__ __launch_bounds__(64) void k_n2v_loss_grad(const float *__restrict__ emb, long long N, int D, const long long *__restrict__ rows,
                                                      long long R, int len, int C, int negative, double scale, double *__restrict__ loss_acc,
                                                      float *__restrict__ grad, unsigned char *__restrict__ touched) {
    extern __shared__ float n2v_smem[];
    const int DP = D + 1, W = len + 1 - C, CM = C - 1, P = W * CM;
    float *__restrict__ E = n2v_smem;
    float *__restrict__ coef = E + (size_t)len * DP;
    float *__restrict__ T = coef + P;                               // [N2V_SLOTS][D] merged gradient rows
    int *__restrict__ ids = reinterpret_cast<int *>(T + (size_t)N2V_SLOTS * D);
    int *__restrict__ keys = ids + len;                             // node of slot s, s < used
    const int lane = threadIdx.x;
    int used = 0;                                                    // wave-uniform
    double wave_loss = 0.0;
    const long long r_begin = (long long)blockIdx.x * N2V_ROWS_PER_WAVE, r_end = min(R, r_begin + N2V_ROWS_PER_WAVE);
    for (long long r = r_begin; r < r_end; ++r) {
        __syncthreads();                                             // the previous row's LDS is no longer read
        bool ok = true;
        for (int i = lane; i < len; i += 64) {
            const long long v = rows[r * len + i];
            ok = ok && v >= 0 && v < N;
            ids[i] = (int)v;
        }
        __syncthreads();
        if (__any(!ok)) continue;                                    // a node id outside the table: the row contributes nothing (wave-uniform)
        for (int i = 0; i < len; ++i) {
            const float *__restrict__ src = emb + (size_t)ids[i] * D;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int d = lane + 64 * k;
                if (d < D) E[i * DP + d] = src[d];
            }
        }
        __syncthreads();
        // one (window j, context slot k) pair per lane: out = <emb[w_j], emb[w_{j+k}]>
        for (int p = lane; p < P; p += 64) {
            const int j = p / CM, k = p % CM + 1;
            const float *__restrict__ a = E + j * DP, *__restrict__ b = E + (j + k) * DP;
            double s0 = 0.0, s1 = 0.0;
            for (int d = 0; d < D; d += 2) {                         // D is even
                s0 += (double)a[d] * (double)b[d];
                s1 += (double)a[d + 1] * (double)b[d + 1];
            }
            const double out = s0 + s1;
            const double sg = 1.0 / (1.0 + exp(-out));
            // term = -log(q + 1e-15) with q = sigmoid(out) or 1 - sigmoid(out); d term / d out = -+ sigmoid (1 - sigmoid) / (q + 1e-15)
            const double q = (negative ? 1.0 - sg : sg) + 1e-15;
            wave_loss += -log(q);
            const double dq = sg * (1.0 - sg);
            coef[p] = (float)(scale * (negative ? dq : -dq) / q);
        }
        if (grad) {
            __syncthreads();
            for (int i = 0; i < len; ++i) {
                float g[NK];
#pragma unroll
                for (int k = 0; k < NK; ++k) g[k] = 0.f;
                if (i < W) {                                         // position i starts window i: its contexts are i + 1 .. i + C - 1
                    for (int k = 1; k <= CM; ++k) {
                        const float c = coef[i * CM + k - 1];
                        const float *__restrict__ e = E + (i + k) * DP;
#pragma unroll
                        for (int m = 0; m < NK; ++m) {
                            const int d = lane + 64 * m;
                            if (d < D) g[m] += c * e[d];
                        }
                    }
                }
                for (int k = 1; k <= CM; ++k) {                      // position i is context slot k of window i - k
                    const int j = i - k;
                    if (j < 0 || j >= W) continue;
                    const float c = coef[j * CM + k - 1];
                    const float *__restrict__ e = E + j * DP;
#pragma unroll
                    for (int m = 0; m < NK; ++m) {
                        const int d = lane + 64 * m;
                        if (d < D) g[m] += c * e[d];
                    }
                }
                const int v = ids[i];
                const unsigned long long hit = __ballot(lane < used && keys[lane] == v);
                int slot = hit ? __ffsll((long long)hit) - 1 : -1;
                const bool fresh = !hit && used < N2V_SLOTS;
                if (fresh) {
                    slot = used++;
                    if (lane == 0) keys[slot] = v;
                }
                if (slot >= 0) {                                     // this wave alone owns T: plain LDS read-modify-write
#pragma unroll
                    for (int m = 0; m < NK; ++m) {
                        const int d = lane + 64 * m;
                        if (d < D) T[slot * D + d] = fresh ? g[m] : T[slot * D + d] + g[m];
                    }
                    __syncthreads();                                 // keys[slot] is read by the next position's lookup
                } else {                                             // no slot left: straight to memory
                    float *__restrict__ dst = grad + (size_t)v * D;
#pragma unroll
                    for (int m = 0; m < NK; ++m) {
                        const int d = lane + 64 * m;
                        if (d < D) atomicAdd(dst + d, g[m]);         // 256 contiguous bytes per wave-instruction
                    }
                    if (lane == 0) touched[v] = 1;
                }
            }
        }
    }
    if (grad) {
        __syncthreads();
        for (int s = 0; s < used; ++s) {
            const int v = keys[s];
            float *__restrict__ dst = grad + (size_t)v * D;
#pragma unroll
            for (int m = 0; m < NK; ++m) {
                const int d = lane + 64 * m;
                if (d < D) atomicAdd(dst + d, T[s * D + d]);         // 256 contiguous bytes per wave-instruction
            }
            if (lane == 0) touched[v] = 1;
        }
    }
    wave_loss = wave_sum(wave_loss);
    if (lane == 0 && wave_loss != 0.0) atomicAdd(loss_acc, scale * wave_loss);
}

// torch.optim.SparseAdam on the flagged rows:
//   m += (g - m) (1 - beta1);  v += (g g - v) (1 - beta2);  p += -step_size * (m / (sqrt(v) + eps)),  step_size = lr sqrt(1 - beta2^t) / (1 - beta1^t)
// Every operation written above is ONE float32 operation, rounded once to nearest, in that order.  `fp contract(off)` keeps the compiler
// from fusing a multiply into the add or subtract that follows it (the default, -ffp-contract=fast, fused g g - v, v + (..)(1 - beta2)
// and p + step * upd: one rounding where the formula has two).  sqrtf is the correctly rounded root (v_sqrt_f32, then the neighbour
// below and the one above tried with an exact FMA residual); __fsqrt_rn compiled to v_sqrt_f32 alone, which is within 1 ulp and not
// always the nearest.  The division is the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence.
// tests/test_node2vec_loss_gpu.py compares the three tables bit for bit with a NumPy float32 restatement of these lines.
//
// One BLOCK per group of 64 flags: each of its 4 waves reads the same 64 flags and takes every fourth flagged row.  A wave works through
// its rows one after the other, each a chain of dependent loads and ALU instructions, and at N = 19 717 a launch with one wave per
// group left about one wave on each CU, so the kernel ran at the speed of that chain: the unfused operations and the root's two trials
// added 3.8 us to its 54 us; with the rows dealt to four waves it takes 23 us.  Rows are independent: the same bits.
template <int NK>
__global__ __launch_bounds__(256) void k_n2v_sparse_adam(float *__restrict__ p, float *__restrict__ grad, unsigned char *__restrict__ touched,
                                                         float *__restrict__ m1, float *__restrict__ m2, long long N, int D, float neg_step_size,
                                                         float one_minus_b1, float one_minus_b2, float eps) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    for (long long base = (long long)blockIdx.x * 64; base < N; base += (long long)gridDim.x * 64) {   // block-uniform trip count
        const long long mine = base + lane;
        const bool flag = mine < N && touched[mine] != 0;
        u64 mask = __ballot(flag);                                   // the same 64 flags in each of the block's 4 waves
        __syncthreads();                                             // all four have read them
        if (wib == 0 && flag) touched[mine] = 0;
        for (int rank = 0; mask; ++rank) {                           // flagged row number `rank` of the group goes to wave rank % 4
            const int b = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            if ((rank & 3) != wib) continue;
            const size_t row = (size_t)(base + b) * D;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int d = lane + 64 * k;
                if (d < D) {
                    const size_t o = row + d;
                    const float g = grad[o], m = m1[o], v = m2[o];
                    const float mn = m + (g - m) * one_minus_b1;
                    const float vn = v + (g * g - v) * one_minus_b2;
                    const float root = sqrtf(vn);
                    const float upd = mn / (root + eps);
                    m1[o] = mn;
                    m2[o] = vn;
                    p[o] = p[o] + neg_step_size * upd;
                    grad[o] = 0.f;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Deterministic mode: contributions stored per walk position, then summed per node in entry order -- no float atomics.
// ------------------------------------------------------------------------------------------------
// k_n2v_loss_grad's LDS without the merged rows (their keys' 64 bytes stay in the formula: one formula, one term dropped).
__host__ __device__ inline size_t n2v_position_lds_bytes(int len, int C, int D) {
    return n2v_lds_bytes(len, C, D) - (size_t)N2V_SLOTS * (size_t)D * sizeof(float);
}

// One wave per row; the arithmetic of k_n2v_loss_grad up to and including g[].  What leaves is a pure function of (emb, the row):
// nothing depends on R, on the grid or on another row.
template <int NK>
__global__ __launch_bounds__(64) void k_n2v_position_grads(const float *__restrict__ emb, long long N, int D, const long long *__restrict__ rows,
                                                           int len, int C, int negative, double scale, int *__restrict__ ids_out,
                                                           float *__restrict__ contrib, double *__restrict__ row_loss) {
    extern __shared__ float n2v_smem[];
    const int DP = D + 1, W = len + 1 - C, CM = C - 1, P = W * CM;
    float *__restrict__ E = n2v_smem;
    float *__restrict__ coef = E + (size_t)len * DP;
    int *__restrict__ ids = reinterpret_cast<int *>(coef + P);
    const int lane = threadIdx.x;
    const long long r = blockIdx.x;
    bool ok = true;
    for (int i = lane; i < len; i += 64) {
        const long long v = rows[r * len + i];
        ok = ok && v >= 0 && v < N;
        ids[i] = (int)v;
    }
    __syncthreads();
    ok = !__any(!ok);                                                // a node id outside the table: the row contributes nothing (wave-uniform)
    for (int i = lane; i < len; i += 64) ids_out[r * len + i] = ok ? ids[i] : -1;
    if (!ok) {
        if (lane == 0) row_loss[r] = 0.0;
        return;
    }
    for (int i = 0; i < len; ++i) {
        const float *__restrict__ src = emb + (size_t)ids[i] * D;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int d = lane + 64 * k;
            if (d < D) E[i * DP + d] = src[d];
        }
    }
    __syncthreads();
    double loss = 0.0;
    for (int p = lane; p < P; p += 64) {                             // one (window j, context slot k) pair per lane, as in k_n2v_loss_grad
        const int j = p / CM, k = p % CM + 1;
        const float *__restrict__ a = E + j * DP, *__restrict__ b = E + (j + k) * DP;
        double s0 = 0.0, s1 = 0.0;
        for (int d = 0; d < D; d += 2) {
            s0 += (double)a[d] * (double)b[d];
            s1 += (double)a[d + 1] * (double)b[d + 1];
        }
        const double out = s0 + s1;
        const double sg = 1.0 / (1.0 + exp(-out));
        const double q = (negative ? 1.0 - sg : sg) + 1e-15;
        loss += -log(q);
        const double dq = sg * (1.0 - sg);
        coef[p] = (float)(scale * (negative ? dq : -dq) / q);
    }
    loss = wave_sum(loss);                                       // a butterfly: the same pattern whatever the row
    if (lane == 0) row_loss[r] = loss;
    __syncthreads();
    for (int i = 0; i < len; ++i) {
        float g[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) g[k] = 0.f;
        if (i < W) {                                                 // position i starts window i: its contexts are i + 1 .. i + C - 1
            for (int k = 1; k <= CM; ++k) {
                const float c = coef[i * CM + k - 1];
                const float *__restrict__ e = E + (i + k) * DP;
#pragma unroll
                for (int m = 0; m < NK; ++m) {
                    const int d = lane + 64 * m;
                    if (d < D) g[m] += c * e[d];
                }
            }
        }
        for (int k = 1; k <= CM; ++k) {                              // position i is context slot k of window i - k
            const int j = i - k;
            if (j < 0 || j >= W) continue;
            const float c = coef[j * CM + k - 1];
            const float *__restrict__ e = E + j * DP;
#pragma unroll
            for (int m = 0; m < NK; ++m) {
                const int d = lane + 64 * m;
                if (d < D) g[m] += c * e[d];
            }
        }
        float *__restrict__ dst = contrib + ((size_t)r * len + i) * D;
#pragma unroll
        for (int m = 0; m < NK; ++m) {
            const int d = lane + 64 * m;
            if (d < D) dst[d] = g[m];                                // 256 contiguous bytes per wave-instruction
        }
    }
}

constexpr int N2V_AHEAD = 8;
constexpr int N2V_SCAN_THREADS = 1024;                            // the one block of k_n2v_loss_sum

__global__ __launch_bounds__(256) void k_n2v_det_clear(int *__restrict__ start, long long N) {
    det_clear_body(start, N, (long long)blockIdx.x * blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
}

// The producer of det_index.h's slots.  FILL = false: start[v] = entries that name node v.  FILL = true (start[v] = first slot of v's
// list): every entry puts itself into the list of its node.
template <bool FILL>
__global__ __launch_bounds__(256) void k_n2v_det_index(const int *__restrict__ ids, int M, long long N, int *__restrict__ start,
                                                       int *__restrict__ list) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < M; e += (long long)gridDim.x * blockDim.x) {
        const int v = ids[e];
        if (v < 0 || v >= N) continue;
        const int at = atomicAdd(&start[v], 1);
        if (FILL && at >= 0 && at < M) list[at] = (int)e;
    }
}

__global__ __launch_bounds__(DET_SCAN_THREADS) void k_n2v_det_scan(int *__restrict__ start, long long N) { det_scan_body(start, N); }

// acc += (double)contrib[e] for the `cnt` entries e the lanes hold (lane t: the t-th), strictly in lane order.  N2V_AHEAD rows are
// loaded before the first addition of a round; past the end the last row is loaded again and not added.
template <int NK>
__device__ __forceinline__ void n2v_add_rows(const int entry, const int cnt, const float *__restrict__ contrib, const int D, const int lane,
                                             double (&acc)[NK]) {
    for (int t0 = 0; t0 < cnt; t0 += N2V_AHEAD) {
        float r[N2V_AHEAD][NK];
#pragma unroll
        for (int u = 0; u < N2V_AHEAD; ++u) {
            const float *row = contrib + (size_t)__shfl(entry, min(t0 + u, cnt - 1)) * D;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int d = lane + 64 * k;
                r[u][k] = d < D ? row[d] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < N2V_AHEAD; ++u) {
            if (t0 + u < cnt) {
#pragma unroll
                for (int k = 0; k < NK; ++k) acc[k] = acc[k] + (double)r[u][k];
            }
        }
    }
}

// Lists longer than a wave, sorted: one thread per list slot p ranks its entry against its whole list (rank = the entries below it;
// entries are distinct) and writes it to sorted[beg + rank].  Quadratic in the list's length, but spread over len / 64 waves: a list
// of 26 880 entries (a hub) took 1.1 s when the one wave that sums it ranked it alone.  Slots of lists up to 64 entries leave at once.
__global__ __launch_bounds__(256) void k_n2v_det_rank(const int *__restrict__ ids, const int *__restrict__ start, const int *__restrict__ list,
                                                      int *__restrict__ sorted, int M, long long N) {
    const int total = min(max(start[N - 1], 0), M);                  // the end of the last list: the slots the fill wrote
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x) {
        const int mine = list[p];
        if ((unsigned)mine >= (unsigned)M) continue;
        const int v = ids[mine];
        if (v < 0 || v >= N) continue;
        int beg, end;
        det_list_bounds(start, v, total, beg, end);
        if (end - beg <= 64 || p < beg || p >= end) continue;
        int rank = 0;
        for (int m = beg; m < end; ++m) {
            const int o = list[m];
            rank += det_ranks_before(o, mine, m, p) ? 1 : 0;
        }
        sorted[beg + rank] = mine;                                   // rank <= end - beg - 1: the entry itself is never counted
    }
}

// grad[v] = (float)((double)grad[v] + sum over v's list, in ascending entry order, of (double)contrib[e]); touched[v] = 1.  One wave per
// node with a list (D <= 256: one 256-column slab); a node without entries is neither read nor written.  A list of up to 64 entries
// is sorted in registers; a longer one is read from `sorted`, where k_n2v_det_rank left it in order.  Every entry read from the index
// is range-checked before it addresses contrib.
template <int NK>
__global__ __launch_bounds__(256) void k_n2v_sum_det(const int *__restrict__ start, const int *__restrict__ list, const int *__restrict__ sorted,
                                                     int M, long long N,
                                                     const float *__restrict__ contrib, int D, float *__restrict__ grad,
                                                     unsigned char *__restrict__ touched) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long v = wave; v < N; v += nwaves) {
        int beg, end;
        det_list_bounds(start, v, M, beg, end);
        const int len = end - beg;
        if (len == 0) continue;
        double acc[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) acc[k] = 0.0;
        if (len <= 64) {
            int entry = lane < len ? list[beg + lane] : 0x7fffffff;
            entry = wave_sort_ascending(entry, lane);
            if ((unsigned)entry >= (unsigned)M) entry = 0;            // (the lanes past the list)
            n2v_add_rows<NK>(entry, len, contrib, D, lane, acc);
        } else {
            for (int p0 = 0; p0 < len; p0 += 64) {
                const int cnt = min(64, len - p0);
                int entry = lane < cnt ? sorted[beg + p0 + lane] : 0;
                if ((unsigned)entry >= (unsigned)M) entry = 0;
                n2v_add_rows<NK>(entry, cnt, contrib, D, lane, acc);
            }
        }
        float *__restrict__ dst = grad + (size_t)v * D;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int d = lane + 64 * k;
            if (d < D) dst[d] = (float)((double)dst[d] + acc[k]);    // one rounding to float32
        }
        if (lane == 0) touched[v] = 1;
    }
}

// *loss_acc += scale * S, S = the float64 sum of row_loss[0 .. R): thread t adds rows t, t + 1024, ... in order, a butterfly per wave,
// then the 16 wave sums in order -- a function of R alone.  One block, one plain add: the adds of a stream land in stream order.
__global__ __launch_bounds__(N2V_SCAN_THREADS) void k_n2v_loss_sum(const double *__restrict__ row_loss, long long R, double scale,
                                                                   double *__restrict__ loss_acc) {
    __shared__ double s_wave[N2V_SCAN_THREADS / 64];
    double v = 0.0;
    for (long long r = threadIdx.x; r < R; r += N2V_SCAN_THREADS) v += row_loss[r];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < N2V_SCAN_THREADS / 64; ++w) s += s_wave[w];
        *loss_acc += scale * s;
    }
}

static bool n2v_dim_ok(int D) { return D >= 32 && D <= 256 && D % 32 == 0; }

// The index of pope_n2v_accumulate_det inside its scratch (det_index.h: start [N + 1] | list [M] | sorted [M]).  0: sizes it refuses (or M == 0).
static size_t n2v_det_scratch_bytes(int64_t M, int64_t N) {
    if (M <= 0 || N < 1 || N >= (1ll << 31) || M >= INT32_MAX) return 0;
    return ((size_t)(N + 1) + 2 * (size_t)M) * sizeof(int);
}

}  // namespace pope

using namespace pope;

extern "C" int pope_n2v_walks(const int32_t *rowptr, const int32_t *col, int64_t N, const int64_t *starts, int64_t B, int64_t B_neg,
                              int32_t walk_length, uint64_t seed, int64_t first_row, int64_t *pos, int64_t *neg, void *stream_) {
    clear_error();
    POPE_REQUIRE(N >= 1 && N < (1ll << 31), "pope_n2v_walks: need 1 <= N < 2^31, got %lld", (long long)N);
    POPE_REQUIRE(walk_length >= 1, "pope_n2v_walks: need walk_length >= 1, got %d", walk_length);
    POPE_REQUIRE(B >= 0 && B_neg >= 0 && B_neg <= B && first_row >= 0,
                 "pope_n2v_walks: need 0 <= B_neg <= B and first_row >= 0 (negative row i starts at starts[i] too)");
    POPE_REQUIRE(B == 0 || (starts && (pos || B_neg > 0) && (!pos || (rowptr && col))), "pope_n2v_walks: null pointer");
    POPE_REQUIRE(B_neg == 0 || neg, "pope_n2v_walks: null pointer (neg with B_neg > 0)");
    const long long B_pos = pos ? B : 0;                              // pos == NULL: negative rows only
    if (B_pos + B_neg == 0) return POPE_OK;
    hipLaunchKernelGGL(k_n2v_walks, dim3(capped_grid((size_t)(B_pos + B_neg), 256)), dim3(256), 0, (hipStream_t)stream_, rowptr, col, (long long)N,
                       (const long long *)starts, B_pos, (long long)B_neg, walk_length, (u64)seed, (long long)first_row, (long long *)pos,
                       (long long *)neg);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" int pope_n2v_walks_biased(const int32_t *rowptr, const int32_t *col, int64_t N, const int64_t *starts, int64_t B,
                                     int32_t walk_length, uint64_t seed, int64_t first_row, double p, double q, int64_t *pos, void *stream_) {
    clear_error();
    POPE_REQUIRE(N >= 1 && N < (1ll << 31), "pope_n2v_walks_biased: need 1 <= N < 2^31, got %lld", (long long)N);
    POPE_REQUIRE(walk_length >= 1, "pope_n2v_walks_biased: need walk_length >= 1, got %d", walk_length);
    POPE_REQUIRE(B >= 0 && first_row >= 0, "pope_n2v_walks_biased: need B >= 0 and first_row >= 0");
    POPE_REQUIRE(std::isfinite(p) && std::isfinite(q) && p > 0.0 && q > 0.0, "pope_n2v_walks_biased: need finite p > 0 and q > 0, got p = %g, q = %g",
                 p, q);
    POPE_REQUIRE(B == 0 || (rowptr && col && starts && pos), "pope_n2v_walks_biased: null pointer");
    if (B == 0) return POPE_OK;
    const double inv_p = 1.0 / p, inv_q = 1.0 / q, w_max = fmax(fmax(inv_p, 1.0), inv_q);
    hipLaunchKernelGGL(k_n2v_walks_biased, dim3(capped_grid((size_t)B * 64, 256)), dim3(256), 0, (hipStream_t)stream_, rowptr, col, (long long)N,
                       (const long long *)starts, (long long)B, walk_length, (u64)seed, (long long)first_row, inv_p, inv_q, w_max,
                       (long long *)pos);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" int pope_n2v_windows(const int64_t *rows, int64_t R, int32_t len, int32_t context, int64_t *windows, void *stream_) {
    clear_error();
    POPE_REQUIRE(R >= 0 && len >= 2, "pope_n2v_windows: need R >= 0 and len >= 2");
    POPE_REQUIRE(context >= 2 && context <= len, "pope_n2v_windows: need 2 <= context <= len, got context %d, len %d", context, len);
    POPE_REQUIRE(R == 0 || (rows && windows), "pope_n2v_windows: null pointer");
    if (R == 0) return POPE_OK;
    hipLaunchKernelGGL(k_n2v_windows, dim3(capped_grid((size_t)R * (size_t)(len + 1 - context) * (size_t)context, 256)), dim3(256), 0,
                       (hipStream_t)stream_, (const long long *)rows, (long long)R, len, context, (long long *)windows);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" int pope_n2v_loss_grad(const float *emb, int64_t N, int32_t D, const int64_t *rows, int64_t R, int32_t len, int32_t context,
                                  int32_t negative, double scale, double *loss_acc, float *grad, uint8_t *touched, void *stream_) {
    clear_error();
    POPE_REQUIRE(N >= 1 && N < (1ll << 31) && R >= 0, "pope_n2v_loss_grad: need 1 <= N < 2^31 and R >= 0");
    POPE_REQUIRE(n2v_dim_ok(D), "pope_n2v_loss_grad: D must be a multiple of 32 from 32 to 256, got %d", D);
    POPE_REQUIRE(len >= 2 && context >= 2 && context <= len, "pope_n2v_loss_grad: need 2 <= context <= len, got context %d, len %d", context,
                 len);
    const size_t lds = n2v_lds_bytes(len, context, D);
    POPE_REQUIRE(lds <= 64u * 1024u, "pope_n2v_loss_grad: a row of %d nodes at D = %d needs %zu bytes of LDS (limit 65536)", len, D, lds);
    POPE_REQUIRE(emb && loss_acc && (R == 0 || rows), "pope_n2v_loss_grad: null pointer");
    POPE_REQUIRE(!grad || touched, "pope_n2v_loss_grad: null pointer (touched with grad)");
    if (R == 0) return POPE_OK;
    const long long blocks_ll = (R + N2V_ROWS_PER_WAVE - 1) / N2V_ROWS_PER_WAVE;
    POPE_REQUIRE(blocks_ll < (1ll << 31), "pope_n2v_loss_grad: too many rows (%lld)", (long long)R);
    const unsigned blocks = (unsigned)blocks_ll;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), lds, (hipStream_t)stream_, emb, (long long)N, D, (const long long *)rows, (long long)R,
                           len, context, negative ? 1 : 0, scale, loss_acc, grad, touched);
    };
    switch ((D + 63) / 64) {
        case 1: launch(k_n2v_loss_grad<1>); break;
        case 2: launch(k_n2v_loss_grad<2>); break;
        case 3: launch(k_n2v_loss_grad<3>); break;
        default: launch(k_n2v_loss_grad<4>); break;
    }
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" int pope_n2v_position_grads(const float *emb, int64_t N, int32_t D, const int64_t *rows, int64_t R, int32_t len, int32_t context,
                                       int32_t negative, double scale, int32_t *ids, float *contrib, double *row_loss, void *stream_) {
    clear_error();
    POPE_REQUIRE(N >= 1 && N < (1ll << 31) && R >= 0, "pope_n2v_position_grads: need 1 <= N < 2^31 and R >= 0");
    POPE_REQUIRE(n2v_dim_ok(D), "pope_n2v_position_grads: D must be a multiple of 32 from 32 to 256, got %d", D);
    POPE_REQUIRE(len >= 2 && context >= 2 && context <= len, "pope_n2v_position_grads: need 2 <= context <= len, got context %d, len %d",
                 context, len);
    const size_t lds = n2v_position_lds_bytes(len, context, D);
    POPE_REQUIRE(lds <= 64u * 1024u, "pope_n2v_position_grads: a row of %d nodes at D = %d needs %zu bytes of LDS (limit 65536)", len, D, lds);
    POPE_REQUIRE(R == 0 || (emb && rows && ids && contrib && row_loss), "pope_n2v_position_grads: null pointer");
    POPE_REQUIRE(R < (1ll << 31), "pope_n2v_position_grads: too many rows (%lld)", (long long)R);
    if (R == 0) return POPE_OK;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)R), dim3(64), lds, (hipStream_t)stream_, emb, (long long)N, D, (const long long *)rows, len,
                           context, negative ? 1 : 0, scale, ids, contrib, row_loss);
    };
    switch ((D + 63) / 64) {
        case 1: launch(k_n2v_position_grads<1>); break;
        case 2: launch(k_n2v_position_grads<2>); break;
        case 3: launch(k_n2v_position_grads<3>); break;
        default: launch(k_n2v_position_grads<4>); break;
    }
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" size_t pope_n2v_accumulate_det_scratch_bytes(int64_t M, int64_t N) { return n2v_det_scratch_bytes(M, N); }

extern "C" int pope_n2v_accumulate_det(const int32_t *ids, int64_t M, const float *contrib, int32_t D, int64_t N, float *grad, uint8_t *touched,
                                       const double *row_loss, int64_t R, double scale, double *loss_acc, void *scratch, size_t scratch_bytes,
                                       void *stream_) {
    clear_error();
    POPE_REQUIRE(N >= 1 && N < (1ll << 31) && M >= 0 && M < INT32_MAX && R >= 0,
                 "pope_n2v_accumulate_det: need 1 <= N < 2^31, 0 <= M < 2^31 - 1 and R >= 0");
    POPE_REQUIRE(n2v_dim_ok(D), "pope_n2v_accumulate_det: D must be a multiple of 32 from 32 to 256, got %d", D);
    const bool with_loss = row_loss && R > 0;
    POPE_REQUIRE(M == 0 || (ids && contrib && grad && touched && scratch), "pope_n2v_accumulate_det: null pointer");
    POPE_REQUIRE(!with_loss || loss_acc, "pope_n2v_accumulate_det: null pointer (loss_acc with row_loss)");
    const size_t need = n2v_det_scratch_bytes(M, N);
    if (scratch_bytes < need) {
        set_error("pope_n2v_accumulate_det: scratch %zu < %zu bytes", scratch_bytes, need);
        return POPE_ERR_WORKSPACE;
    }
    if (M == 0 && !with_loss) return POPE_OK;
    hipStream_t stream = (hipStream_t)stream_;
    if (M > 0) {
        int *start = static_cast<int *>(scratch), *list = start + (N + 1), *sorted = list + M;
        const dim3 entries(capped_grid((size_t)M, 256));
        hipLaunchKernelGGL(k_n2v_det_clear, dim3(capped_grid((size_t)N + 1, 256)), dim3(256), 0, stream, start, (long long)N);
        hipLaunchKernelGGL(k_n2v_det_index<false>, entries, dim3(256), 0, stream, ids, (int)M, (long long)N, start, list);
        hipLaunchKernelGGL(k_n2v_det_scan, dim3(1), dim3(DET_SCAN_THREADS), 0, stream, start, (long long)N);
        hipLaunchKernelGGL(k_n2v_det_index<true>, entries, dim3(256), 0, stream, ids, (int)M, (long long)N, start, list);
        hipLaunchKernelGGL(k_n2v_det_rank, entries, dim3(256), 0, stream, ids, (const int *)start, (const int *)list, sorted, (int)M, (long long)N);
        const dim3 nodes(capped_grid((size_t)N * 64, 256));
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, nodes, dim3(256), 0, stream, (const int *)start, (const int *)list, (const int *)sorted, (int)M, (long long)N,
                               contrib, D, grad, touched);
        };
        switch ((D + 63) / 64) {
            case 1: launch(k_n2v_sum_det<1>); break;
            case 2: launch(k_n2v_sum_det<2>); break;
            case 3: launch(k_n2v_sum_det<3>); break;
            default: launch(k_n2v_sum_det<4>); break;
        }
    }
    if (with_loss) hipLaunchKernelGGL(k_n2v_loss_sum, dim3(1), dim3(N2V_SCAN_THREADS), 0, stream, row_loss, (long long)R, scale, loss_acc);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" int pope_n2v_sparse_adam(float *emb, float *grad, uint8_t *touched, float *exp_avg, float *exp_avg_sq, int64_t N, int32_t D,
                                    double lr, double beta1, double beta2, double eps, int64_t step, void *stream_) {
    clear_error();
    POPE_REQUIRE(N >= 0 && N < (1ll << 31), "pope_n2v_sparse_adam: need 0 <= N < 2^31");
    POPE_REQUIRE(n2v_dim_ok(D), "pope_n2v_sparse_adam: D must be a multiple of 32 from 32 to 256, got %d", D);
    POPE_REQUIRE(step >= 1 && lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
                 "pope_n2v_sparse_adam: need step >= 1, lr >= 0, 0 <= beta < 1, eps >= 0");
    POPE_REQUIRE(N == 0 || (emb && grad && touched && exp_avg && exp_avg_sq), "pope_n2v_sparse_adam: null pointer");
    if (N == 0) return POPE_OK;
    // scalars in double, as Python forms them for torch.optim.SparseAdam, rounded to float once
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const float neg_step_size = (float)(-(lr * sqrt(bc2) / bc1));
    const unsigned blocks = capped_grid((size_t)((N + 63) / 64) * 256, 256, 256u * 8u);       // one block per 64 flags
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, emb, grad, touched, exp_avg, exp_avg_sq, (long long)N, D,
                           neg_step_size, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps);
    };
    switch ((D + 63) / 64) {
        case 1: launch(k_n2v_sparse_adam<1>); break;
        case 2: launch(k_n2v_sparse_adam<2>); break;
        case 3: launch(k_n2v_sparse_adam<3>); break;
        default: launch(k_n2v_sparse_adam<4>); break;
    }
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}
