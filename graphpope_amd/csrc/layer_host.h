// What the whole-graph layers (sage_full.h, gcn.h, gat.h, gatv2.h) share on the host (included in place in sage.hip, ahead of them).
// The rule: a conv call's launches -- their order and the conditions under which each happens -- are written ONCE, as a function template
// over a sink.  The entry point walks the list with a LaunchRun, which enqueues; the call's *_kernel_name query walks the same list with a
// LaunchNames, which appends each launch's printed name.  Every step is one statement that holds both the name and the launch, and a
// templated kernel's instantiation and its name are formed side by side from the same booleans, so what is printed is what runs.
// No kernel lives here: the device side of the hub list stays with each layer.
#pragma once

namespace pope {

inline const char *tf(bool b) { return b ? "true" : "false"; }

// The printed name of one launch: a format and up to four strings for it (template arguments, by tf()).
struct KName { const char *fmt, *a = "", *b = "", *c = "", *d = ""; };

// The answer of a *_kernel_name query: the launches in order, joined by '+'.
struct NameBuf {
    char buf[1536];
    int n = 0;

    template <class... A>
    void add(const char *fmt, A... args) {
        if (n < (int)sizeof buf) n += snprintf(buf + n, sizeof buf - n, "%s", n ? "+" : "");
        if (n < (int)sizeof buf) n += snprintf(buf + n, sizeof buf - n, fmt, args...);
    }
    // launch_gemm's launches: the tile kernel as instantiated, and k_slab_reduce behind split depth
    void add_gemm(GemmTile t, GemmLayouts l, int splits) {
        const int wm = t.tm == 128 ? 4 : 2, wn = t.tm == 128 ? 1 : 2;
        if (splits > 1) add("k_gemm<%d, %d, %d, %d, %d, %d>[splits=%d]+k_slab_reduce", t.tm, t.tn, wm, wn, (int)l.a, (int)l.b, splits);
        else add("k_gemm<%d, %d, %d, %d, %d, %d>", t.tm, t.tn, wm, wn, (int)l.a, (int)l.b);
    }
    int copy_to(const char *who, char *name, size_t cap) const {
        POPE_REQUIRE((size_t)n < cap && n < (int)sizeof buf, "%s: %d characters do not fit name[%zu]", who, n, cap);
        memcpy(name, buf, (size_t)n + 1);
        return POPE_OK;
    }
};

// The sink that runs a launch list.  The first step that fails ends it: every step behind is skipped, and done() returns that error.
struct LaunchRun {
    void *scratch;
    hipStream_t stream;
    int cus;
    int rc = POPE_OK;

    float *floats(size_t offset) const { return scratch_at<float>(scratch, offset); }
    int *ints(size_t offset) const { return scratch_at<int>(scratch, offset); }
    template <class... P, class... A>
    void launch(const KName &, void (*kernel)(P...), dim3 grid, dim3 block, A... args) {
        if (!rc) hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
    }
    void gemm(const GemmArgs &p, GemmTile tile, GemmLayouts layouts) {
        if (!rc) rc = launch_gemm(p, tile, layouts, stream);
    }
    // C [M, N] = A [M, K] B [N, K]^T (+ bias) in whole tiles of 16 rb rows (gemm_tile16.h)
    void tile16(const float *A, const float *B, int K, int M, int N, const float *bias, float *C, int rb) {
        if (!rc) rc = gemm_tile16(A, B, K, nullptr, nullptr, 0, K, K, M, N, bias, C, N, rb, cus, stream, nullptr, nullptr);
    }
    // out [C] = the column sums of g [rows, C]: row slices into part [COLSUM_SPLITS, C], then the slices in order
    void colsum(const float *g, int rows, int C, float *part, bool vec, float *out) {
        if (rc) return;
        enqueue_colsum_partial(g, rows, C, part, nullptr, vec, stream);
        hipLaunchKernelGGL(k_colsum_final, dim3((C + 15) / 16), dim3(256), 0, stream, part, COLSUM_SPLITS, C, out);
    }
    int done() const {                   // what the entry point returns behind its list
        if (rc) return rc;
        POPE_HIP(hipGetLastError());
        return POPE_OK;
    }
};

// The sink that names it: no pointer it hands out or is given is followed.
struct LaunchNames {
    int cus;
    NameBuf names;

    float *floats(size_t) const { return nullptr; }
    int *ints(size_t) const { return nullptr; }
    template <class... P, class... A>
    void launch(const KName &k, void (*)(P...), dim3, dim3, A...) { names.add(k.fmt, k.a, k.b, k.c, k.d); }
    void gemm(const GemmArgs &p, GemmTile tile, GemmLayouts layouts) { names.add_gemm(tile, layouts, p.gz); }
    void tile16(const float *, const float *, int, int, int, const float *, float *, int rb) { names.add("k_gemm_tile16<%d, %d>", rb, t16_buffers()); }
    void colsum(const float *, int, int, float *, bool vec, float *) { names.add("k_colsum_partial<%s>+k_colsum_final", tf(vec)); }
};

static int scratch_too_small(const char *who, size_t have, size_t need) {
    set_error("%s: scratch %zu < %zu bytes", who, have, need);
    return POPE_ERR_WORKSPACE;
}

// ---- the hub list (the layout: gcn.h's GcnHubScratch, or sage_full.h's own; both name their members alike) ----
template <class Args, class Sink, class Layout>
static void hub_bind(Args &a, const Sink &s, const Layout &lay) {
    a.counters = s.ints(lay.counters); a.hubs = s.ints(lay.hubs); a.chunks = s.ints(lay.chunks); a.partial = s.floats(lay.partial);
    a.hub_cap = lay.hub_cap; a.chunk_cap = lay.chunk_cap;
}

// The row sums over [N, width] rows: the counters cleared by `clear` (null: the caller has cleared them), one wave per (row, 256-column
// slab), and with hubs the two launches behind it, sized by capacity.  `tail`: what the rows and the partial kernel take behind the args.
template <class Sink, class Args, class... Tail>
static void hub_family(Sink &s, bool hubs, void (*clear)(int *), const Args &a, int width, const KName &rows_name, void (*rows)(Args, Tail...),
                       const KName &partial_name, void (*partial)(Args, Tail...), const KName &finish_name, void (*finish)(Args), Tail... tail) {
    const int slabs = (width + 255) / 256;
    if (hubs && clear) s.launch(KName{"k_gcn_clear"}, clear, dim3(1), dim3(64), a.counters);
    // at least `slabs` waves, and a multiple of four of them: every slab has its waves
    s.launch(rows_name, rows, dim3(std::max(capped_grid((size_t)a.N * slabs * 64, 256), (unsigned)(slabs + 3) / 4)), dim3(256), a, tail...);
    if (!hubs) return;
    s.launch(partial_name, partial, dim3(capped_grid((size_t)a.chunk_cap * slabs * 64, 256)), dim3(256), a, tail...);
    s.launch(finish_name, finish, dim3(capped_grid((size_t)a.hub_cap * slabs * 64, 256)), dim3(256), a);
}

// ---- the dense parts ----
// out [M, n_out] = x [M, c_in] W^T (+ bias): whole tiles with rb (W.p then [n_out, c_in], depth-contiguous), else the plain tile kernel.
template <class Sink>
static void project(Sink &s, const float *x, int c_in, int M, int n_out, const Operand &W, const float *bias, float *out, int rb, GemmTile tile,
                   GemmLayouts layouts) {
    if (rb) return s.tile16(x, W.p, c_in, M, n_out, bias, out, rb);
    GemmArgs p = gemm_problem(Operand{x, c_in, 1}, W, c_in, M, n_out, out, n_out);
    p.bias = bias;
    s.gemm(p, tile, layouts);
}

// out [m, n] = A [depth, m]^T B [depth, n], the depth in `splits` slices through `slab` (a weight gradient: depth = the graph's rows).
template <class Sink>
static void split_depth_gemm(Sink &s, const float *A, int m, const float *B, int n, int depth, float *out, int splits, float *slab, GemmTile tile,
                             GemmLayouts layouts) {
    GemmArgs p = gemm_problem(Operand{A, 1, m}, Operand{B, 1, n}, depth, m, n, out, n);
    p.gz = splits; p.slab = slab;
    s.gemm(p, tile, layouts);
}

}  // namespace pope
