"""Shapes, inputs and float64 references shared by tests/test_sage_backward_gpu.py (which runs them on the device) and tests/test_abi.py
(which pins the kernel path of every shape on the CPU and checks that the exact family's sums stay exact).  Not a test module.

A layer is (n_dst, c_in, c_out) plus `extra` = n_src - n_dst.  PATHS says which launches sage_backward_kernel_name must report for it on
256 CUs with both optional gradients wanted: the shapes were picked as the smallest that reach each path, so a retune that moves one of
them must fail the pin instead of silently testing another path.

Inputs.  Exact family: small integers stored as float32 (G in [-3, 3], agg and x in [-4, 4], W in [-2, 2]) and row degrees from
{0, 1, 2, 4, 8, 128}: every product, partial sum and atomic sum is an integer or a multiple of 2^-7 below 2^24, so float32 additions in
any order give the same bits and the comparison has no tolerance.  Rounding family: randn gradients and weights, [0, 1) features, degrees
0 .. 9, compared within a derived bound (Reference.bounds).

Extents.  Buffers are allocated at the capacity; past the true sizes the inputs hold poison that is safe to read: NaN rows, and indices
that stay inside their allocation but point at NaN rows / at output rows that must keep their sentinel."""
import functools

import numpy as np
import scipy.sparse as sp

SENTINEL = 12345.0
CUS = 256

STREAMK = "k_gemm_streamk_tn<32>%s+k_streamk_tn_fixup<32>"
T64, T128, T256 = "64, 64, 2, 2", "64, 128, 2, 2", "128, 256, 4, 1"
GENERIC, OC_OC, KC_OC = "0, 0", "2, 2", "1, 2"

# (n_dst, c_in, c_out): (weight-gradient path, splits, weight-gradient tile, grad_x tile, layouts "vec" / "generic")
PATHS = {
    (4065, 256, 256): ("streamk_xcd", 0, None, T64, "vec"),        # first depth that qualifies (tiles_m = 4) ...
    (4064, 256, 256): ("dual", 16, None, None, "vec"),             # ... and its neighbour
    (4160, 256, 256): ("streamk_xcd", 0, None, T64, "vec"),        # the capacity of the extent cases
    (16500, 512, 64): ("streamk_xcd", 0, None, T256, "vec"),       # tiles_m = 1, grad_x on the 128 x 256 twin
    (4100, 260, 68): ("streamk_xcd", 0, None, T128, "vec"),        # c_in / c_out tails: M - 4 clamp, second column panel of 4
    (1700, 260, 260): ("streamk", 0, None, T64, "vec"),            # plain deal, tiles_m = 5
    (5500, 256, 192): ("streamk", 0, None, T64, "vec"),            # plain deal, tiles_m = 3
    (2100, 756, 256): ("streamk_xcd", 0, None, T128, "vec"),       # layer 0 (run without grad_x, plain and indexed)
    (1030, 40, 24): ("dual", 5, T64, T64, "vec"),                  # (tiles: of the twin path it takes when dual is refused)
    (257, 64, 64): ("dual", 2, None, None, "vec"),
    (600, 516, 8): ("dual", 3, None, None, "vec"),
    (256, 64, 64): ("twin", 1, T64, T64, "vec"),
    (1, 4, 4): ("twin", 1, T64, T64, "vec"),
    (515, 37, 30): ("twin", 3, T64, T64, "generic"),
    (300, 130, 257): ("twin", 2, T64, T64, "generic"),
    (130, 7, 3): ("twin", 1, T64, T64, "generic"),
    (5, 7, 3): ("twin", 1, T64, T64, "generic"),
    (6500, 132, 250): ("twin", 25, T128, T128, "generic"),
}


def expected_name(shape, extra, grad_x=True, grad_b=True, xcd=True):
    """What sage_backward_kernel_name must print for `shape` with n_src = n_dst + extra: the format of include/graphpope_hip.h filled in
    from PATHS (a table of outcomes, not a restatement of the thresholds)."""
    path, splits, w_tile, x_tile, lay = PATHS[shape]
    if path == "dual" and grad_x and grad_b:
        return "k_gemm_dual<64, 64, 2, 2>[splits=%d]+k_scatter_and_finals" % splits
    vec = lay == "vec"
    colsum = "k_colsum_partial<%s>" % ("true" if vec else "false")
    parts = []
    if path.startswith("streamk"):
        if grad_b:
            parts.append(colsum)
        parts.append(STREAMK % ("[xcd]" if path == "streamk_xcd" and xcd else ""))
    else:
        gemm = "k_gemm<%s, %s>" % (w_tile, OC_OC if vec else GENERIC)
        parts.append(gemm + ("[splits=%d]+k_slab_reduce" % splits if splits > 1 else ""))
        if grad_b:
            parts.append(colsum + "+k_colsum_final")
    if grad_x:
        if extra > 0:
            parts.append("k_zero_rows")
        parts.append("k_gemm<%s, %s>" % (x_tile, KC_OC if vec else GENERIC))
        parts.append("k_scatter_mean")
    return "+".join(parts)


def _case(shape, extra=0, grad_x=True, grad_b=True, indexed=False, edges=True, xcd=True, trues=None, family="exact"):
    name = "%dx%d-%d+%d" % (shape + (extra,))
    name += ("" if grad_x else "-nogx") + ("" if grad_b else "-nogb") + ("-indexed" if indexed else "") + ("" if edges else "-nnz0")
    name += ("" if xcd else "-xcd0") + ("-true" + "_".join(map(str, trues)) if trues else "") + ("" if family == "exact" else "-" + family)
    return dict(id=name, shape=shape, extra=extra, grad_x=grad_x, grad_b=grad_b, indexed=indexed, edges=edges, xcd=xcd, trues=trues,
                family=family)


def _host_cases():
    out = []
    for shape in PATHS:
        if shape == (2100, 756, 256):                                  # layer 0: no input gradient, through both entry points
            out += [_case(shape, extra, grad_x=False, indexed=ix) for extra in (0, 300) for ix in (False, True)]
            continue
        out += [_case(shape, extra) for extra in (0, 300)]
    for extra in (0, 300):
        out += [_case((1030, 40, 24), extra, grad_b=False), _case((1030, 40, 24), extra, grad_x=False),  # dual refused: OC-layout twin
                _case((1030, 40, 24), extra, grad_x=False, indexed=True)]                                # ... behind k_gather_rows
        # no edges, once per family (dual: the k_bwd_finals branch)
        out += [_case(s, extra, edges=False) for s in ((4160, 256, 256), (1030, 40, 24), (256, 64, 64), (515, 37, 30))]
        # the plain deal at the shapes that take the XCD-aware one by default
        out += [_case(s, extra, xcd=False) for s in PATHS if PATHS[s][0] == "streamk_xcd" and s != (2100, 756, 256)]
        out += [_case((2100, 756, 256), extra, grad_x=False, indexed=ix, xcd=False) for ix in (False, True)]
    return out


def _extent_cases():
    """(true n_dst values, the larger first) under a capacity: every run of a case reuses the buffers, scratch included, of the one before."""
    table = [
        ((4160, 256, 256), (4129, 1000, 700), {}),          # tail stage of 1 row; units = blocks; 44 units for 64 quads
        ((16500, 512, 64), (4200, 1500), {}),               # (1500: fewer units than quads)
        ((1700, 260, 260), (1669, 600), {}),
        ((2100, 756, 256), (2069, 700), dict(grad_x=False)),
        ((2100, 756, 256), (2069, 700), dict(grad_x=False, indexed=True)),
        ((1030, 40, 24), (999, 300), {}),
        ((515, 37, 30), (484, 130), {}),
        ((1030, 40, 24), (999, 300), dict(grad_x=False, indexed=True)),
    ]
    out = []
    for shape, trues, kw in table:
        out += [_case(shape, extra, trues=trues, **kw) for extra in (0, 300)]
        if PATHS[shape][0] == "streamk_xcd":
            out += [_case(shape, extra, trues=trues, xcd=False, **kw) for extra in (0, 300)]
    return out


# one shape per path
ROUNDING_CASES = [_case(s, extra, family="rounding", **kw) for s, kw in (
    ((4160, 256, 256), {}), ((16500, 512, 64), {}), ((1700, 260, 260), {}), ((2100, 756, 256), dict(grad_x=False, indexed=True)),
    ((1030, 40, 24), {}), ((1030, 40, 24), dict(grad_b=False)), ((515, 37, 30), {}), ((6500, 132, 250), {})) for extra in (0, 300)]
ROUNDING_CASES += [_case((4160, 256, 256), extra, trues=(700,), family="rounding") for extra in (0, 300)]
HOST_CASES = _host_cases()
EXTENT_CASES = _extent_cases()

# The layer shapes of the benchmark (B = 1 550, fan-outs [25, 10], 756 -> 256 -> 256): a sampled batch and the capacities of
# the device-extent step.  (n_dst, n_src, c_in, c_out, grad_x): name
BASELINE_NAMES = {
    (9988, 104000, 756, 256, False): "k_colsum_partial<true>+" + STREAMK % "[xcd]",
    (40300, 443300, 756, 256, False): "k_colsum_partial<true>+" + STREAMK % "[xcd]",
    (40300, 443300, 256, 256, True): "k_colsum_partial<true>+" + STREAMK % "[xcd]" + "+k_zero_rows+k_gemm<%s, %s>+k_scatter_mean" % (T256, KC_OC),
    (1550, 10136, 256, 256, True): "k_gemm_dual<64, 64, 2, 2>[splits=7]+k_scatter_and_finals",
    (1550, 40300, 256, 256, True): "k_gemm_dual<64, 64, 2, 2>[splits=7]+k_scatter_and_finals",
}


def size_query_args():
    """(n_src, n_dst, nnz, c_in, c_out) of every layer in HOST_CASES, EXTENT_CASES and BASELINE_NAMES, each once: the arguments at which
    tests/golden/sage_scratch_sizes.json pins the scratch size queries (nnz: any count that is no multiple of an alignment)."""
    layers = [(c["shape"][0] + c["extra"],) + c["shape"] for c in HOST_CASES + EXTENT_CASES]
    layers += [(n_src, n_dst, c_in, c_out) for n_dst, n_src, c_in, c_out, _ in BASELINE_NAMES]
    return [(n_src, n_dst, 5 * n_dst + 3, c_in, c_out) for n_src, n_dst, c_in, c_out in sorted(set(layers))]


class Reference:
    """Inputs of one run at its true sizes and the float64 results of the operation written out:
        grad_w_l = G^T agg    grad_w_r = G^T x_dst    grad_b = colsum G
        grad_x[:n] = G W_r    grad_x[col[p]] += (G W_l)[i] / deg_i   for every edge p of row i
    (for the exact family every one of these float64 values is the exact sum, whatever the order)."""

    def __init__(self, n, n_src, c_in, c_out, family, edges, seed):
        rs = np.random.RandomState(seed)
        self.n, self.n_src, self.c_in, self.c_out, self.family = n, n_src, c_in, c_out, family
        if family == "exact":
            deg = rs.choice([0, 1, 2, 4, 8], size=n)
            deg[rs.choice(n, size=min(3, n), replace=False)] = 128       # the scatter's 64-neighbour chunk loop runs twice
            ints = lambda lo, hi, *shape: rs.randint(lo, hi + 1, size=shape).astype(np.float32)
            self.g, self.agg, self.x = ints(-3, 3, n, c_out), ints(-4, 4, n, c_in), ints(-4, 4, n, c_in)
            self.w_l, self.w_r = ints(-2, 2, c_out, c_in), ints(-2, 2, c_out, c_in)
        else:
            deg = rs.randint(0, 10, size=n)
            self.g = rs.randn(n, c_out).astype(np.float32)
            self.agg, self.x = rs.rand(n, c_in).astype(np.float32), rs.rand(n, c_in).astype(np.float32)
            self.w_l, self.w_r = (rs.randn(c_out, c_in) * 0.5).astype(np.float32), (rs.randn(c_out, c_in) * 0.5).astype(np.float32)
        if not edges:
            deg[:] = 0
        self.deg = deg
        self.rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
        self.nnz = int(self.rowptr[-1])
        self.col = rs.randint(0, n_src, size=self.nnz).astype(np.int32)
        # mean[j, i] = (edges i -> j) / deg_i in float64 (exact for the power-of-two degrees of the exact family)
        inv = np.repeat(1.0 / np.maximum(deg, 1), deg)
        self.mean_t = sp.csr_matrix((inv, self.col.astype(np.int64), self.rowptr.astype(np.int64)), shape=(n, n_src)).T.tocsr()
        self.in_deg = np.bincount(self.col, minlength=n_src)

    @staticmethod
    def _results(g, agg, x, w_l, w_r, mean_t, n, n_src):
        gx = np.zeros((n_src, x.shape[1]))
        gx[:n] = g @ w_r
        gx += mean_t @ (g @ w_l)
        return dict(grad_w_l=g.T @ agg, grad_w_r=g.T @ x, grad_b=g.sum(axis=0), grad_x=gx)

    @functools.cached_property
    def want(self):
        f = lambda a: a.astype(np.float64)
        return self._results(f(self.g), f(self.agg), f(self.x), f(self.w_l), f(self.w_r), self.mean_t, self.n, self.n_src)

    @functools.cached_property
    def magnitude(self):
        """The same expressions on absolute values: a bound on every partial sum, in any order."""
        f = lambda a: np.abs(a.astype(np.float64))
        return self._results(f(self.g), f(self.agg), f(self.x), f(self.w_l), f(self.w_r), self.mean_t, self.n, self.n_src)

    def assert_exact_family_is_exact(self):
        """Every partial sum of the weight and bias gradients is an integer below 2^24 and every partial sum of grad_x a multiple of 2^-7
        below 2^17: float32 represents them all, so no addition rounds."""
        assert self.family == "exact" and set(np.unique(self.deg)) <= {0, 1, 2, 4, 8, 128}
        m = self.magnitude
        assert max(m["grad_w_l"].max(), m["grad_w_r"].max(), m["grad_b"].max()) < 2 ** 24
        assert 128 * m["grad_x"].max() < 2 ** 24
        assert np.array_equal(self.want["grad_x"] * 128, np.round(self.want["grad_x"] * 128))

    def bounds(self):
        """Rounding family.  A float32 sum of n terms in any order, each term one rounded product, is within (n + 1) u of the exact sum
        times the sum of absolute values (u = 2^-24; to first order, the slack below covers the rest): the weight and bias gradients add
        n_true terms, through at most two more roundings where partial sums are combined -- (n_true + 3) u.  A term of grad_x[j, c] passes
        through at most c_out + 1 roundings in the GEMM, one in the multiplication by 1 / deg (itself one rounding of 1 / deg: the + 4),
        and the d_j atomic additions of row j: (c_out + d_j + 4) u."""
        u = 2.0 ** -24
        m = self.magnitude
        out = {k: (self.n + 3) * u * m[k] for k in ("grad_w_l", "grad_w_r", "grad_b")}
        out["grad_x"] = (self.c_out + self.in_deg[:, None] + 4) * u * m["grad_x"]
        return out


def true_sizes(case, n):
    """(n_src_true, capacities n_dst, n_src) of a run of `case` with n true destination rows (n = capacity for a host-sized run)."""
    cap = case["shape"][0]
    n_src_cap = cap + case["extra"]
    if n == cap:
        return n_src_cap, cap, n_src_cap
    # with n_src == n_dst as capacities no row is zeroed for the scatter alone: the true sizes then are equal too
    return (n + case["extra"] // 2), cap, n_src_cap


def reference_key(case, n):
    """What the inputs of a run of `case` with n true rows depend on: two runs with the same key share their Reference."""
    _, c_in, c_out = case["shape"]
    n_src_true, _, _ = true_sizes(case, n)
    return n, n_src_true, c_in, c_out, case["family"], case["edges"]


def reference(case, n):
    return _reference(*reference_key(case, n))


@functools.lru_cache(maxsize=3)
def _reference(n, n_src, c_in, c_out, family, edges):
    return Reference(n, n_src, c_in, c_out, family, edges, seed=n + 7 * c_in + 13 * c_out)


# ---- poison past the true sizes (both directions) ----
def nan_padded(a, total):
    """`a` followed by NaN rows up to `total` rows."""
    out = np.full((total, a.shape[1]), np.nan, dtype=np.float32)
    out[:len(a)] = a
    return out


def padded_csr(rowptr, col, n_cap, nnz_cap, lo, hi, rs):
    """The block at its capacities: rows past the true count are empty (rowptr = nnz, as the sampler writes it) and the entries of col
    past nnz are indices in [lo, hi) -- rows that hold poison or a sentinel (0 where there are none: lo >= hi)."""
    nnz = len(col)
    rp = np.full(n_cap + 1, nnz, dtype=np.int32)
    rp[:len(rowptr)] = rowptr
    cl = rs.randint(lo, hi, size=max(nnz_cap, 1)).astype(np.int32) if lo < hi else np.zeros(max(nnz_cap, 1), dtype=np.int32)
    cl[:nnz] = col
    return rp, cl


def indexed_rows(x, n_rows, n_id_len, c_in, rs):
    """A feature matrix of n_rows rows that is NaN except at n_id[:len(x)], where it holds x; n_id (n_id_len entries, distinct)."""
    n_id = rs.permutation(n_rows)[:n_id_len].astype(np.int64)
    feats = np.full((n_rows, c_in), np.nan, dtype=np.float32)
    feats[n_id[:len(x)]] = x
    return feats, n_id


# ---- forward, extents only ----
# ((capacity n_dst, c_in, c_out), knob set to 0 or None, the kernels sage_forward_kernel_name reports on 256 CUs): the four forms of the
# projection.  4160 rows are stream-K under every setting; 5800 is the smallest capacity of test_abi's table that takes the overlapped form.
FORWARD = [
    ((4160, 256, 256), None, "k_gemm_streamk_ld<32>"),
    ((4160, 256, 256), "KNOB_SAGE_FORWARD_OVERLAP", "k_gemm_streamk_ld<32>"),
    ((4160, 256, 256), "KNOB_FORWARD_WHOLE_TILES", "k_gemm_streamk_ld<32>"),
    ((5800, 256, 256), None, "k_gather_beside_gemm<3>+k_gemm_tile16<3, 4>"),
    ((5800, 256, 256), "KNOB_SAGE_FORWARD_OVERLAP", "k_gemm_tile16<3, 4>"),
    ((5800, 256, 256), "KNOB_FORWARD_WHOLE_TILES", "k_gemm_streamk_ld<32>"),
    ((13312, 48, 48), None, "k_gemm_tile16<4, 4>"),
    ((515, 37, 30), None, "k_gemm<64, 64>"),
]
FORWARD_EXTRA = 300                                                    # n_src - n_dst of the capacities


def forward_trues(cap):
    """True destination counts under a capacity, the larger first."""
    return (cap - 31, 700 if cap > 700 else 130)


class ForwardReference:
    """Exact-family inputs of a forward run with n true destinations and n + 150 true sources, and the float64 results
        agg[i] = mean over row i of x[col[p]]      out = agg W_l^T + b + x[:n] W_r^T."""

    def __init__(self, n, c_in, c_out):
        rs = np.random.RandomState(n + c_in)
        self.n, self.n_src = n, n + FORWARD_EXTRA // 2
        self.deg = rs.choice([0, 1, 2, 4, 8], size=n)
        self.deg[rs.choice(n, size=3, replace=False)] = 128
        self.rowptr = np.concatenate([[0], np.cumsum(self.deg)]).astype(np.int32)
        self.nnz = int(self.rowptr[-1])
        ints = lambda lo, hi, *shape: rs.randint(lo, hi + 1, size=shape).astype(np.float32)
        self.x, self.w_l, self.w_r, self.b = ints(-4, 4, self.n_src, c_in), ints(-2, 2, c_out, c_in), ints(-2, 2, c_out, c_in), ints(-2, 2, c_out)
        self.col = rs.randint(0, self.n_src, size=self.nnz).astype(np.int32)
        f = lambda a: a.astype(np.float64)
        inv = np.repeat(1.0 / np.maximum(self.deg, 1), self.deg)
        mean = sp.csr_matrix((inv, self.col.astype(np.int64), self.rowptr.astype(np.int64)), shape=(n, self.n_src))
        self.agg = mean @ f(self.x)
        self.out = self.agg @ f(self.w_l).T + f(self.b) + f(self.x)[:n] @ f(self.w_r).T
        self.magnitude = (mean @ np.abs(f(self.x))) @ np.abs(f(self.w_l)).T + np.abs(f(self.b)) + np.abs(f(self.x))[:n] @ np.abs(f(self.w_r)).T

    def assert_exact_family_is_exact(self):
        """Every partial sum of agg and of out is a multiple of 2^-7 below 2^17: float32 adds them in any order without rounding."""
        assert set(np.unique(self.deg)) <= {0, 1, 2, 4, 8, 128} and 128 * self.magnitude.max() < 2 ** 24
        assert np.array_equal(self.out * 128, np.round(self.out * 128)) and np.array_equal(self.agg * 128, np.round(self.agg * 128))


@functools.lru_cache(maxsize=2)
def forward_reference(n, c_in, c_out):
    return ForwardReference(n, c_in, c_out)
