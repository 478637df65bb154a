// Multinomial / binomial logistic regression on embedding rows: the objective scikit-learn's lbfgs path minimises, and its predictions.
//
// Replaces what PyG's Node2Vec.test does on the host for the model /root/reference/generate_node2vec_embedding.py:23-25 constructs:
// LogisticRegression(solver='lbfgs').fit(train_z, train_y).score(test_z, test_y).  The optimiser stays scipy's L-BFGS-B on the host
// (graphpope_amd/logreg.py); what it calls a few dozen times per fit -- one pass over z for the loss and the gradient -- is here.
//
//   k_logreg_rows<RP>          one wave per row, lanes along d (lane l owns the columns l, l + 64, ...).  z is widened to float64 on
//                              load; a lane keeps one float64 partial product per class in registers, a butterfly per class makes
//                              raw = z W^T + b whole in every lane, and every lane then evaluates the row -- softmax around the row
//                              maximum, or the four-branch binomial form -- identically.  Lane c stores the residual (P - Y)[i, c]
//                              (rows padded with zeros to RP = R rounded up to 1, 4, 8, 16, 32 or 64),
//                              lane 0 the row loss.  A block stages W in LDS once, transposed, where it fits 64 KB; else W is read in place.
//   k_logreg_grad_partial<RP>  the skinny product residual^T [z | 1], split over slices of LOGREG_SLICE_ROWS rows.  A block takes one
//                              slice and 64 columns: lane = column, so a row of z is read coalesced and the residuals of a row are
//                              wave-uniform; each of the 8 waves sums 32 rows of the slice in row order, wave 0 adds the eight
//                              in wave order (through LDS) and stores the float64 partial.  The blocks of the first 64 columns
//                              also sum their slice's row losses.
//   k_logreg_final             one thread per gradient element: the partials in slice order, / m, + l2 w off the intercept column;
//                              one more block: the slices' loss sums in a fixed order, / m, + l2 / 2 |W|^2.
//   k_logreg_predict<RP>       k_logreg_rows' raw, then the first index of the row maximum (np.argmax's rule) or raw > 0; hits
//                              against an encoded y are counted per wave and leave as one INTEGER atomic add per wave.
//
// There is no float atomic and no reduction whose order depends on timing: loss and gradient are pure functions of the inputs, bit
// for bit, on every call.  A row's raw, residual and loss depend on that row's z and on w alone, and the gradient's summation order
// on the row POSITION alone, so rows selected through ids give the bits of the same rows materialised.
#include <cmath>
#include <type_traits>

#include "common.h"
#include "wave.h"

namespace pope {

static constexpr int LOGREG_MAX_CLASSES = 64;
static constexpr int LOGREG_SLICE_ROWS = 256;          // rows per float64 partial of the gradient's first stage
static constexpr int LOGREG_THREADS = 256;
static constexpr int LOGREG_GRAD_THREADS = 512;          // the gradient's first stage: 8 waves x 32 rows of a slice
static constexpr int LOGREG_GRAD_UNROLL = 8;
static constexpr size_t LOGREG_LDS_BYTES = 64u * 1024u;
static constexpr unsigned LOGREG_ROW_BLOCKS = 256u * 8u;     // the row kernels' grid cap: a block stages W once for all its rows

// The wave's index in its block, as a value the compiler knows to be the same in every lane: what is indexed by it (row ids, labels,
// residuals) is then read with scalar loads, several in flight, instead of one vector load at a time.
__device__ __forceinline__ int logreg_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// max that keeps a NaN (fmax would drop it)
__device__ __forceinline__ double logreg_max(double a, double b) { return (a > b || a != a) ? a : b; }

// W as a block reads it: element (class c, column j) at base[c * sc + j * sj].
struct LogregW {
    const double *base;
    int sc, sj;
};

// Where R (d + icpt) doubles fit the 64 KB of LDS a block may take, the block keeps W there TRANSPOSED ([c][j]: the lanes of a wave,
// which own consecutive columns, read consecutive words); else every wave reads it in place (j * R + c: L1 / L2 hits, strided).
__device__ __forceinline__ LogregW logreg_stage_w(const double *__restrict__ w, int R, int cols, int in_lds, double *s_w) {
    if (!in_lds) return {w, 1, R};
    for (int e = threadIdx.x; e < R * cols; e += LOGREG_THREADS) s_w[(e % R) * cols + e / R] = w[e];
    __syncthreads();
    return {s_w, cols, 1};
}

// raw[c] = <z row, W[c]> + b[c] for c < R, the same bits in every lane.  zrow == nullptr (an id outside the table): NaN.
template <int RP>
__device__ __forceinline__ void logreg_raw(const float *__restrict__ zrow, int d, int R, int icpt, const LogregW w, int lane,
                                           double (&raw)[RP]) {
#pragma unroll
    for (int c = 0; c < RP; ++c) raw[c] = 0.0;
    if (zrow) {
        for (int j = lane; j < d; j += 64) {
            const double zj = (double)zrow[j];
            const double *wj = w.base + (size_t)j * w.sj;
#pragma unroll
            for (int c = 0; c < RP; ++c) raw[c] += zj * wj[(c < R ? c : R - 1) * w.sc];   // no branch around a load: c >= R repeats class R - 1, unused
        }
    }
#pragma unroll
    for (int c = 0; c < RP; ++c) {
        if (c < R) {
            raw[c] = wave_sum(raw[c]);
            if (icpt) raw[c] += w.base[(size_t)d * w.sj + c * w.sc];
            if (!zrow) raw[c] = NAN;
        }
    }
}

__device__ __forceinline__ const float *logreg_row(const float *__restrict__ z, long long ldz, long long N, const long long *__restrict__ ids,
                                                   long long i) {
    const long long row = ids ? ids[i] : i;
    return row >= 0 && row < N ? z + row * ldz : nullptr;
}

template <int RP>
__global__ __launch_bounds__(LOGREG_THREADS) void k_logreg_rows(const float *__restrict__ z, long long ldz, long long N,
                                                                 const long long *__restrict__ ids, long long m, int d,
                                                                 const int *__restrict__ y, int R, int icpt, int w_in_lds,
                                                                 const double *__restrict__ w_global, double *__restrict__ res,
                                                                 double *__restrict__ row_loss) {
    extern __shared__ double s_w[];
    const LogregW w = logreg_stage_w(w_global, R, d + icpt, w_in_lds, s_w);
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (LOGREG_THREADS / 64);
    for (long long i = (long long)blockIdx.x * (LOGREG_THREADS / 64) + logreg_wave(); i < m; i += waves) {
        double raw[RP];
        logreg_raw<RP>(logreg_row(z, ldz, N, ids, i), d, R, icpt, w, lane, raw);
        const int yi = y[i];
        double loss, mine = 0.0;
        if constexpr (RP == 1) {
            // HalfBinomialLoss: log(1 + exp(raw)) - y raw and sigmoid(raw) - y, in the branches of scikit-learn's closs_grad_half_binomial
            const double x = raw[0], yt = yi == 1 ? 1.0 : 0.0;
            double g;
            if (x <= -37.0) {
                g = exp(x);
                loss = g - yt * x;
                g -= yt;
            } else if (x <= -2.0) {
                g = exp(x);
                loss = log1p(g) - yt * x;
                g = ((1.0 - yt) * g - yt) / (1.0 + g);
            } else if (x <= 18.0) {
                g = exp(-x);
                loss = log1p(g) + (1.0 - yt) * x;
                g = ((1.0 - yt) - yt * g) / (1.0 + g);
            } else {                                                   // a NaN lands here and stays one
                g = exp(-x);
                loss = g + (1.0 - yt) * x;
                g = ((1.0 - yt) - yt * g) / (1.0 + g);
            }
            mine = g;
        } else {
            // HalfMultinomialLoss: logsumexp(raw) - raw[y] and softmax(raw) - onehot(y), around the row maximum
            double mx = raw[0];
#pragma unroll
            for (int c = 1; c < RP; ++c)
                if (c < R) mx = logreg_max(mx, raw[c]);
            double own = 0.0, raw_y = 0.0;                             // lane c takes class c: one exponential and one quotient per lane
#pragma unroll
            for (int c = 0; c < RP; ++c) {
                if (c < R) {
                    if (lane == c) own = raw[c];
                    if (c == yi) raw_y = raw[c];
                }
            }
            const double e = lane < R ? exp(own - mx) : 0.0;
            double sum = 0.0;
#pragma unroll
            for (int c = 0; c < RP; ++c)
                if (c < R) sum += wave_read_lane(e, c);                   // in class order, the same in every lane
            loss = log(sum) + mx - raw_y;
            mine = e / sum - (lane == yi ? 1.0 : 0.0);
        }
        if (lane < RP) res[i * RP + lane] = lane < R ? mine : 0.0;     // rows of RP: the gradient kernel reads them whole
        if (lane == 0) row_loss[i] = loss;
    }
}

template <int RP>
__global__ __launch_bounds__(LOGREG_GRAD_THREADS) void k_logreg_grad_partial(const float *__restrict__ z, long long ldz, long long N,
                                                                              const long long *__restrict__ ids, long long m, int d, int R,
                                                                              int cols, const double *__restrict__ res,
                                                                              const double *__restrict__ row_loss,
                                                                              double *__restrict__ partial, double *__restrict__ loss_partial) {
    constexpr int WAVES = LOGREG_GRAD_THREADS / 64, WAVE_ROWS = LOGREG_SLICE_ROWS / WAVES;
    __shared__ double s_acc[RP][64];
    __shared__ double s_loss[LOGREG_SLICE_ROWS / 64];
    const int lane = threadIdx.x & 63, wave = logreg_wave();
    if (blockIdx.y == 0) {                                             // the slice's row losses: a butterfly per 64 rows, the sums in order
        const long long r = (long long)blockIdx.x * LOGREG_SLICE_ROWS + threadIdx.x;
        if (threadIdx.x < LOGREG_SLICE_ROWS) {
            const double v = wave_sum(r < m ? row_loss[r] : 0.0);
            if (lane == 0) s_loss[wave] = v;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double v = 0.0;
            for (int k = 0; k < LOGREG_SLICE_ROWS / 64; ++k) v += s_loss[k];
            loss_partial[blockIdx.x] = v;
        }
    }
    const int j = blockIdx.y * 64 + lane;
    const bool active = j < cols;
    const int jz = j < d ? j : d - 1;                                  // the intercept's column reads a value it does not use
    const long long lo = (long long)blockIdx.x * LOGREG_SLICE_ROWS + wave * WAVE_ROWS;
    const long long hi = lo + WAVE_ROWS < m ? lo + WAVE_ROWS : m;
    double acc[RP];
#pragma unroll
    for (int c = 0; c < RP; ++c) acc[c] = 0.0;
    // No branch around a load, and no load left to be sunk into one: the loads of 8 rows are in flight together (a row past the end
    // repeats the wave's last row with a factor 0, a row outside the table reads row 0 with a factor 0 -- its residual is NaN
    // already), and the sums stay in row order.
    static_assert(LOGREG_GRAD_UNROLL == 8, "the barrier below names 8 values");
    auto rows = [&](auto by_id) {
        for (long long i0 = lo; i0 < hi; i0 += LOGREG_GRAD_UNROLL) {
            float v[LOGREG_GRAD_UNROLL];
            bool keep[LOGREG_GRAD_UNROLL];
#pragma unroll
            for (int u = 0; u < LOGREG_GRAD_UNROLL; ++u) {
                const long long i = i0 + u < hi ? i0 + u : hi - 1;
                long long row = i;
                if constexpr (decltype(by_id)::value) row = ids[i];
                const bool inside = row >= 0 && row < N;
                v[u] = z[(inside ? row : 0) * ldz + jz];
                keep[u] = inside && i0 + u < hi;
            }
            asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
#pragma unroll
            for (int u = 0; u < LOGREG_GRAD_UNROLL; ++u) {
                const double zj = j < d ? (keep[u] ? (double)v[u] : 0.0) : (i0 + u < hi ? 1.0 : 0.0);   // j == d: the intercept's column
                const double *ri = res + (i0 + u < hi ? i0 + u : hi - 1) * RP;
#pragma unroll
                for (int c = 0; c < RP; ++c) acc[c] += ri[c] * zj;
            }
        }
    };
    if (active) {
        if (ids) rows(std::true_type{});
        else rows(std::false_type{});
    }
    for (int turn = 1; turn < WAVES; ++turn) {                         // wave 0 += wave 1, 2, ..., in that order
        if (wave == turn) {
#pragma unroll
            for (int c = 0; c < RP; ++c) s_acc[c][lane] = acc[c];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int c = 0; c < RP; ++c) acc[c] += s_acc[c][lane];
        }
        __syncthreads();
    }
    if (wave == 0 && active) {
        double *out = partial + (size_t)blockIdx.x * ((size_t)R * cols) + (size_t)j * R;
#pragma unroll
        for (int c = 0; c < RP; ++c)
            if (c < R) out[c] = acc[c];
    }
}

// Blocks 0 .. gridDim.x - 2: grad[e] = (sum of partial[s][e], s ascending) / m + l2 w[e] (no l2 term in the intercept's column).
// The last block: *loss = (sum of the slices' loss sums) / m + l2 / 2 * sum of w[e]^2 off the intercept's column; thread t adds the
// entries t, t + 256, ... in order, a butterfly per wave, the 4 wave sums in order.
__global__ __launch_bounds__(LOGREG_THREADS) void k_logreg_final(const double *__restrict__ partial, long long slices, long long m, int d, int R,
                                                                  int cols, const double *__restrict__ w, double l2,
                                                                  const double *__restrict__ loss_partial, double *__restrict__ loss,
                                                                  double *__restrict__ grad) {
    const long long P = (long long)R * cols, penalised = (long long)R * d;
    if (blockIdx.x + 1 < gridDim.x) {
        const long long e = (long long)blockIdx.x * LOGREG_THREADS + threadIdx.x;
        if (e >= P) return;
        double s = 0.0;
#pragma unroll 16
        for (long long k = 0; k < slices; ++k) s += partial[k * P + e];
        s /= (double)m;
        if (e < penalised) s += l2 * w[e];
        grad[e] = s;
        return;
    }
    __shared__ double s_wave[2][LOGREG_THREADS / 64];
    double v = 0.0, q = 0.0;
    for (long long k = threadIdx.x; k < slices; k += LOGREG_THREADS) v += loss_partial[k];
    for (long long e = threadIdx.x; e < penalised; e += LOGREG_THREADS) q += w[e] * w[e];
    v = wave_sum(v);
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) {
        s_wave[0][threadIdx.x >> 6] = v;
        s_wave[1][threadIdx.x >> 6] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sv = 0.0, sq = 0.0;
        for (int k = 0; k < LOGREG_THREADS / 64; ++k) {
            sv += s_wave[0][k];
            sq += s_wave[1][k];
        }
        *loss = sv / (double)m + 0.5 * l2 * sq;
    }
}

template <int RP>
__global__ __launch_bounds__(LOGREG_THREADS) void k_logreg_predict(const float *__restrict__ z, long long ldz, long long N,
                                                                    const long long *__restrict__ ids, long long m, int d, int R, int icpt,
                                                                    int w_in_lds, const double *__restrict__ w_global,
                                                                    const int *__restrict__ y, int *__restrict__ pred,
                                                                    unsigned long long *__restrict__ correct) {
    extern __shared__ double s_w[];
    const LogregW w = logreg_stage_w(w_global, R, d + icpt, w_in_lds, s_w);
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (LOGREG_THREADS / 64);
    unsigned long long hits = 0;
    for (long long i = (long long)blockIdx.x * (LOGREG_THREADS / 64) + logreg_wave(); i < m; i += waves) {
        double raw[RP];
        logreg_raw<RP>(logreg_row(z, ldz, N, ids, i), d, R, icpt, w, lane, raw);
        int best = 0;
        if constexpr (RP == 1) {
            best = raw[0] > 0.0 ? 1 : 0;
        } else {
            double top = raw[0];                                       // np.argmax: the first maximum, and a NaN counts as one
#pragma unroll
            for (int c = 1; c < RP; ++c) {
                if (c < R && (raw[c] > top || (raw[c] != raw[c] && top == top))) {
                    top = raw[c];
                    best = c;
                }
            }
        }
        if (lane == 0) {
            pred[i] = best;
            if (y && y[i] == best) ++hits;                             // an unseen label is encoded as -1: never a hit
        }
    }
    if (lane == 0 && hits && correct) atomicAdd(correct, hits);
}

static int logreg_rows_of(int classes) { return classes == 2 ? 1 : classes; }
static int logreg_padded(int R) { return R == 1 ? 1 : R <= 4 ? 4 : R <= 8 ? 8 : R <= 16 ? 16 : R <= 32 ? 32 : 64; }   // RP of LOGREG_DISPATCH

// residual [m, RP] | row_loss [m] | partial [slices, R (d + 1)] | loss_partial [slices], float64 each.  0: extents the calls refuse
// (or m == 0).
static size_t logreg_scratch_bytes(int64_t m, int d, int classes) {
    if (m < 1 || m >= (1ll << 38) || d < 1 || classes < 2 || classes > LOGREG_MAX_CLASSES) return 0;
    const size_t R = (size_t)logreg_rows_of(classes), slices = ((size_t)m + LOGREG_SLICE_ROWS - 1) / LOGREG_SLICE_ROWS;
    return ((size_t)m * logreg_padded((int)R) + (size_t)m + slices * R * ((size_t)d + 1) + slices) * sizeof(double);
}

static int logreg_check_common(const char *who, const float *z, int64_t ldz, int64_t N, int64_t m, int d, int classes, const double *w) {
    POPE_REQUIRE(classes >= 2 && classes <= LOGREG_MAX_CLASSES, "%s: need 2 <= classes <= %d, got %d", who, LOGREG_MAX_CLASSES, classes);
    POPE_REQUIRE(d >= 1, "%s: need d >= 1, got %d", who, d);
    POPE_REQUIRE(ldz >= d, "%s: need ldz >= d, got ldz %lld, d %d", who, (long long)ldz, d);
    POPE_REQUIRE(m >= 0 && m < (1ll << 38) && N >= (m > 0 ? 1 : 0), "%s: need 0 <= m < 2^38 and a table of N >= 1 rows", who);
    POPE_REQUIRE(m == 0 || (z && w), "%s: null pointer", who);
    return POPE_OK;
}

}  // namespace pope

using namespace pope;

extern "C" int32_t pope_logreg_max_classes(void) { return LOGREG_MAX_CLASSES; }
extern "C" int32_t pope_logreg_slice_rows(void) { return LOGREG_SLICE_ROWS; }
extern "C" size_t pope_logreg_scratch_bytes(int64_t m, int32_t d, int32_t classes) { return logreg_scratch_bytes(m, d, classes); }

#define LOGREG_DISPATCH(R, launch, kernel)              \
    do {                                                \
        if ((R) == 1) launch(kernel<1>);                \
        else if ((R) <= 4) launch(kernel<4>);           \
        else if ((R) <= 8) launch(kernel<8>);           \
        else if ((R) <= 16) launch(kernel<16>);         \
        else if ((R) <= 32) launch(kernel<32>);         \
        else launch(kernel<64>);                        \
    } while (0)

extern "C" int pope_logreg_loss_grad(const float *z, int64_t ldz, int64_t N, const int64_t *ids, int64_t m, int32_t d, const int32_t *y,
                                     int32_t classes, int32_t fit_intercept, const double *w, double l2, double *loss, double *grad,
                                     void *scratch, size_t scratch_bytes, void *stream_) {
    clear_error();
    if (int rc = logreg_check_common("pope_logreg_loss_grad", z, ldz, N, m, d, classes, w)) return rc;
    POPE_REQUIRE(m == 0 || (y && loss && grad && scratch), "pope_logreg_loss_grad: null pointer");
    if (m == 0) return POPE_OK;
    const size_t need = logreg_scratch_bytes(m, d, classes);
    POPE_REQUIRE(scratch_bytes >= need, "pope_logreg_loss_grad: scratch of %zu bytes given, %zu needed", scratch_bytes, need);
    POPE_REQUIRE((uintptr_t)scratch % 8 == 0, "pope_logreg_loss_grad: scratch must be 8-byte aligned");
    const int R = logreg_rows_of(classes), icpt = fit_intercept ? 1 : 0, cols = d + icpt;
    const long long slices = (m + LOGREG_SLICE_ROWS - 1) / LOGREG_SLICE_ROWS;
    double *res = (double *)scratch, *row_loss = res + (size_t)m * logreg_padded(R), *partial = row_loss + m;
    double *loss_partial = partial + (size_t)slices * R * ((size_t)d + 1);
    hipStream_t stream = (hipStream_t)stream_;
    const size_t w_bytes = (size_t)R * cols * sizeof(double);
    const int w_in_lds = w_bytes <= LOGREG_LDS_BYTES;
    auto rows = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(capped_grid((size_t)m * 64, LOGREG_THREADS, LOGREG_ROW_BLOCKS)), dim3(LOGREG_THREADS),
                           w_in_lds ? w_bytes : 0, stream, z, (long long)ldz, (long long)N, (const long long *)ids, (long long)m, d, y, R, icpt,
                           w_in_lds, w, res, row_loss);
    };
    LOGREG_DISPATCH(R, rows, k_logreg_rows);
    POPE_HIP(hipGetLastError());
    auto part = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)slices, (unsigned)((cols + 63) / 64)), dim3(LOGREG_GRAD_THREADS), 0, stream, z,
                           (long long)ldz, (long long)N, (const long long *)ids, (long long)m, d, R, cols, (const double *)res,
                           (const double *)row_loss, partial, loss_partial);
    };
    LOGREG_DISPATCH(R, part, k_logreg_grad_partial);
    POPE_HIP(hipGetLastError());
    const long long P = (long long)R * cols;
    hipLaunchKernelGGL(k_logreg_final, dim3((unsigned)((P + LOGREG_THREADS - 1) / LOGREG_THREADS + 1)), dim3(LOGREG_THREADS), 0, stream,
                       (const double *)partial, slices, (long long)m, d, R, cols, w, l2, (const double *)loss_partial, loss, grad);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}

extern "C" int pope_logreg_predict(const float *z, int64_t ldz, int64_t N, const int64_t *ids, int64_t m, int32_t d, int32_t classes,
                                   int32_t fit_intercept, const double *w, const int32_t *y, int32_t *pred, int64_t *correct,
                                   void *stream_) {
    clear_error();
    if (int rc = logreg_check_common("pope_logreg_predict", z, ldz, N, m, d, classes, w)) return rc;
    POPE_REQUIRE(m == 0 || pred, "pope_logreg_predict: null pointer");
    POPE_REQUIRE(!correct || y, "pope_logreg_predict: null pointer (y with correct)");
    hipStream_t stream = (hipStream_t)stream_;
    if (correct && m > 0) POPE_HIP(hipMemsetAsync(correct, 0, sizeof(int64_t), stream));
    if (m == 0) return POPE_OK;
    const int R = logreg_rows_of(classes), icpt = fit_intercept ? 1 : 0;
    const size_t w_bytes = (size_t)R * (d + icpt) * sizeof(double);
    const int w_in_lds = w_bytes <= LOGREG_LDS_BYTES;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(capped_grid((size_t)m * 64, LOGREG_THREADS, LOGREG_ROW_BLOCKS)), dim3(LOGREG_THREADS),
                           w_in_lds ? w_bytes : 0, stream, z, (long long)ldz, (long long)N, (const long long *)ids, (long long)m, d, R, icpt,
                           w_in_lds, w, y, pred, (unsigned long long *)correct);
    };
    LOGREG_DISPATCH(R, launch, k_logreg_predict);
    POPE_HIP(hipGetLastError());
    return POPE_OK;
}
