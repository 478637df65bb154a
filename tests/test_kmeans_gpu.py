"""Every C entry point of csrc/kmeans.hip, called directly, against plain NumPy float64 restatements written in this file.

The end-to-end K-means tests (tests/test_pairwise_gpu.py) judge final centres on separated blobs at depths 16..32; a score
wrong in the fourth digit, a dropped depth tail or a swapped accumulator row still finds the right blob there.  Here every
kernel is compared on unseparated data, at the tile (64 rows x 128 centres), slice (64 deep), block (128 / 256 threads) and
layout (16-byte vector loads / clamped scalar loads) edges, with tolerances DERIVED from the number formats:

  float64 sums        |fl(sum) - sum| <= (n - 1) * 2^-53 * sum|v| for any order; kernel and reference each have one -> n * 2^-52
  float32 dot + score (D + 3) * 2^-24 * (|c|^2 + 2 * sum_k |x_k c_k|): D products and D - 1 additions in any order, the rounding
                      of |c|^2 to float32 and the final FMA
  one rounding        an ulp of the expected float32

Guard bands: every device operand sits inside a larger allocation, 64 elements of sentinel (NaN for floats, the most negative
value for integers, 0xA5 for the scratch bytes) in front and behind; outputs are pre-filled with the sentinel.  After every
call the bands must be bit-identical and no output may be NaN: a clamped load that lets outside data into a result, or a
write past an extent, fails the test without faulting anything.  With `pytest -s` every test prints the fitness of its
input (ambiguous share, seeding margins) next to the cap it has to meet, computed from the reference alone.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64                                   # sentinel elements on either side of every operand (256 for the scratch bytes)
F32_SENTINEL = np.uint32(0x7FC0A5A5)         # a quiet NaN with a payload
F64_SENTINEL = np.uint64(0x7FF8A5A5A5A5A5A5)
U24, U53 = 2.0 ** -24, 2.0 ** -53            # unit roundoffs of float32 / float64


class UnfitInput(Exception):
    """The seeded input does not meet the condition (derived from the reference alone) under which the assertion is exact."""


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


# ---------------------------------------------------------------------------------------------------------------------
# guard bands
# ---------------------------------------------------------------------------------------------------------------------
def _sentinel(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.array([F32_SENTINEL]).view(np.float32)[0]
    if dtype == np.float64:
        return np.array([F64_SENTINEL]).view(np.float64)[0]
    if dtype == np.uint8:
        return np.uint8(0xA5)
    return np.iinfo(dtype).min               # int32 / int64: INT_MIN


class Guarded:
    """`n` elements of `dtype` on the device with GUARD sentinel elements on both sides.  `skew` extra sentinel elements in
    front move the operand off the allocation's 16-byte grid (skew = 1 float: the view starts 4 bytes in)."""

    def __init__(self, dev, dtype, n, values=None, skew=0):
        self.dtype, self.n = np.dtype(dtype), int(n)
        guard = max(GUARD, GUARD * 4 // self.dtype.itemsize)         # at least 256 bytes: the operand keeps the allocation's alignment
        self.lo = guard + skew
        host = np.full(self.lo + self.n + guard, _sentinel(dtype), dtype=self.dtype)
        if values is not None:
            host[self.lo:self.lo + self.n] = np.asarray(values, dtype=self.dtype).reshape(-1)
        self.host0 = host                                            # what the allocation held before the call
        self.buf = torch.as_tensor(host).to(dev)                     # a byte copy: NaN payloads survive
        self.view = self.buf[self.lo:self.lo + self.n]
        assert self.view.data_ptr() % 16 == (skew * self.dtype.itemsize) % 16

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def _download(self):
        return self.buf.cpu().numpy()                                # synchronises with the stream the kernels ran on

    def get(self):
        return self._download()[self.lo:self.lo + self.n].copy()

    def bands_intact(self):
        now = self._download().view(np.uint8)
        was = self.host0.view(np.uint8)
        a, b = self.lo * self.dtype.itemsize, (self.lo + self.n) * self.dtype.itemsize
        return np.array_equal(now[:a], was[:a]) and np.array_equal(now[b:], was[b:])

    def untouched(self):
        return np.array_equal(self._download().view(np.uint8), self.host0.view(np.uint8))


class Bands:
    """All operands of one call: `inp` / `out` / `scratch` allocate, `verify` is the after-call check."""

    def __init__(self, dev):
        self.dev, self.all, self.outputs = dev, {}, {}

    def inp(self, name, values, dtype, skew=0):
        values = np.asarray(values, dtype=dtype)
        g = self.all[name] = Guarded(self.dev, dtype, values.size, values, skew)
        return g

    def out(self, name, dtype, n):
        g = self.all[name] = self.outputs[name] = Guarded(self.dev, dtype, n)
        return g

    def scratch(self, nbytes):
        g = self.all["scratch"] = Guarded(self.dev, np.uint8, nbytes)
        return g

    def verify(self):
        for name, g in self.all.items():
            assert g.bands_intact(), f"guard band of `{name}` was written"
        res = {}
        for name, g in self.outputs.items():
            res[name] = v = g.get()
            if v.dtype.kind == "f":
                assert not np.isnan(v).any(), f"output `{name}` holds NaN (unwritten, or outside data was read)"
            else:
                assert not (v == _sentinel(v.dtype)).any(), f"output `{name}` has unwritten elements"
        return res

    def outputs_untouched(self):
        return all(g.untouched() for g in self.outputs.values())


def _lib():
    from graphpope_amd import _lib as binding
    return binding, binding.load()


def _scratch_bytes(n, d, k):
    return int(_lib()[1].pope_kmeans_scratch_bytes(n, d, k))


def test_scratch_bytes_promise(dev):
    """pope_kmeans_scratch_bytes: 0 for an empty problem, positive otherwise, monotone in every argument over the shapes used
    here (so a buffer sized for a call is sized for every smaller one).  That the promised size is ENOUGH is what every other
    test in this file checks: each gives its call exactly this many bytes between two guard bands."""
    assert _scratch_bytes(0, 4, 4) == 0 and _scratch_bytes(4, 0, 4) == 0 and _scratch_bytes(4, 4, 0) == 0
    base = _scratch_bytes(333, 64, 129)
    assert base > 0
    assert _scratch_bytes(1100, 64, 129) >= base and _scratch_bytes(333, 300, 129) >= base and _scratch_bytes(333, 64, 300) >= base
    # the documented lower bound of pope_column_moments: 256 row slabs x (sum, sum of squares) x D float64
    assert _scratch_bytes(1, 300, 1) >= 256 * 2 * 300 * 8


# ---------------------------------------------------------------------------------------------------------------------
# 1. pope_column_moments / pope_shift_columns
# ---------------------------------------------------------------------------------------------------------------------
MOMENT_SHAPES = [(1, 1), (5, 3), (255, 7), (257, 64), (1000, 128), (300, 300)]   # N across the 256 row slabs, D across the 256-thread block
MOMENT_FAMILIES = {"randn": 0.0, "randn+1000": 1000.0}                           # a large mean: a float32 accumulator would show


def _moment_input(n, d, family):
    rs = np.random.RandomState(n + d)
    return (rs.randn(n, d) + MOMENT_FAMILIES[family]).astype(np.float32)


@pytest.mark.parametrize("family", list(MOMENT_FAMILIES))
@pytest.mark.parametrize("n,d", MOMENT_SHAPES)
def test_column_moments_against_float64(n, d, family, dev):
    """sum[c] and sumsq[c] against X.astype(f64).sum(0) and (X64 ** 2).sum(0).  The kernel accumulates in float64 (the squares
    of float32 values are exact there), so both it and NumPy obey the float64 summation bound (n - 1) * 2^-53 * sum|v| whatever
    their order; together n * 2^-52 of sum|v| (of sum v^2 for the squares) per column."""
    from graphpope_amd import engine
    binding, lib = _lib()
    x = _moment_input(n, d, family)
    b = Bands(dev)
    gx = b.inp("X", x, np.float32)
    gs, gq = b.out("sum", np.float64, d), b.out("sumsq", np.float64, d)
    sc = b.scratch(_scratch_bytes(n, d, 1))
    engine.check(lib.pope_column_moments(gx.ptr, n, d, gs.ptr, gq.ptr, sc.ptr, sc.n, engine._stream()))
    got = b.verify()
    x64 = x.astype(np.float64)
    want_s, want_q = x64.sum(0), (x64 ** 2).sum(0)
    tol_s, tol_q = n * 2.0 ** -52 * np.abs(x64).sum(0), n * 2.0 ** -52 * want_q
    err_s, err_q = np.abs(got["sum"] - want_s), np.abs(got["sumsq"] - want_q)
    print(f"\n[moments {n}x{d} {family}] worst err/tol: sum {np.max(err_s / tol_s):.3g}, sumsq {np.max(err_q / tol_q):.3g} (cap 1)")
    assert (err_s <= tol_s).all() and (err_q <= tol_q).all()


@pytest.mark.parametrize("sign", [-1.0, 1.0])
@pytest.mark.parametrize("family", list(MOMENT_FAMILIES))
@pytest.mark.parametrize("n,d", MOMENT_SHAPES)
def test_shift_columns_is_bit_exact(n, d, family, sign, dev):
    """out = X + sign * shift[column], bit for bit.  The kernel's expression is contracted by the compiler to
    fmaf(sign, shift, X): one rounding.  For sign = -1 and +1, the only values the product path uses, sign * shift is exact,
    so fmaf(sign, shift, X) == np.float32(X) + np.float32(sign) * shift evaluated in float32, and that NumPy expression is
    what is asserted (no tolerance).
    The capped grid (common.h capped_grid: 4096 blocks x 256 threads = 1 048 576 elements in flight) is NOT reachable inside
    this file's size limits (N <= 1 100, D <= 300: at most 330 000 elements), so the grid-stride loop takes one trip here."""
    from graphpope_amd import engine
    binding, lib = _lib()
    x = _moment_input(n, d, family)
    shift = (x.astype(np.float64).mean(0)).astype(np.float32) if sign < 0 else np.random.RandomState(d).randn(d).astype(np.float32)
    b = Bands(dev)
    gx, gsh = b.inp("X", x, np.float32), b.inp("shift", shift, np.float32)
    go = b.out("out", np.float32, n * d)
    engine.check(lib.pope_shift_columns(gx.ptr, gsh.ptr, n, d, sign, go.ptr, engine._stream()))
    got = b.verify()["out"].reshape(n, d)
    want = x + np.float32(sign) * shift[None, :]
    assert want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 2 + 3. pope_kmeans_lloyd_step
# ---------------------------------------------------------------------------------------------------------------------
# N across the 64-row tile; K across one 128-column tile and up to three; D across the 64-deep slice and = 0, 1, 2, 3 mod 4
# (k_assign<LAYOUT_KC_VEC> when D % 4 == 0, k_assign<LAYOUT_GENERIC> otherwise)
LLOYD_SHAPES = [(1, 1, 1), (63, 3, 2), (65, 4, 5), (200, 63, 128), (333, 64, 129), (500, 65, 257), (700, 68, 64), (1100, 128, 300),
                (257, 130, 40), (129, 200, 131)]
SKEWED = (700, 128, 64)                       # D % 4 == 0 but the operands start 4 bytes into their allocations: generic kernel
LLOYD_CASES = [(n, d, k, 0) for n, d, k in LLOYD_SHAPES] + [SKEWED + (1,)]
LLOYD_FAMILIES = {"randn": 0.0, "randn+3": 3.0}   # +3: scores of both signs, cancellation in |c|^2 - 2 x.c
AMBIGUOUS_CAP = 0.05


@functools.lru_cache(maxsize=None)
def _lloyd_input(n, d, k, family, planted):
    """X, C ~ randn (+ offset) from RandomState(N + D + K).  planted: up to two centres (the last one and the middle one, never
    all of them) are moved to 1e6 in every coordinate so that they attract no point."""
    rs = np.random.RandomState(n + d + k)
    off = LLOYD_FAMILIES[family]
    x = (rs.randn(n, d) + off).astype(np.float32)
    c = (rs.randn(k, d) + off).astype(np.float32)
    far = sorted({k - 1, k // 2})[-min(2, k - 1):] if planted and k > 1 else []
    for j in far:
        c[j] = 1e6
    x.setflags(write=False)
    c.setflags(write=False)
    return x, c, tuple(far)


@functools.lru_cache(maxsize=None)
def _assign_reference(n, d, k, family):
    """float64 scores s[i, j] = |c_j|^2 - 2 x_i.c_j, their float32 error bound b[i, j] = (D + 3) 2^-24 (|c_j|^2 + 2 sum_k |x_ik c_jk|),
    the argmin, and per row the set of centres the kernel may legitimately answer: j with s[i, j] <= s[i, best] + b[i, best] + b[i, j]."""
    x, c, _ = _lloyd_input(n, d, k, family, False)
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    c2 = (c64 ** 2).sum(1)
    s = c2[None, :] - 2.0 * (x64 @ c64.T)
    b = (d + 3) * U24 * (c2[None, :] + 2.0 * (np.abs(x64) @ np.abs(c64).T))
    best = s.argmin(1)
    rows = np.arange(n)
    band = s <= (s[rows, best] + b[rows, best])[:, None] + b
    ambiguous = band.sum(1) > 1
    return best, band, ambiguous


def _lloyd_call(dev, x, c, labels_prev, skew=0, short=0):
    """One pope_kmeans_lloyd_step with every operand guarded and exactly the promised scratch (minus `short` bytes)."""
    from graphpope_amd import engine
    binding, lib = _lib()
    (n, d), k = x.shape, c.shape[0]
    b = Bands(dev)
    gx, gc = b.inp("X", x, np.float32, skew), b.inp("centers", c, np.float32, skew)
    gp = b.inp("labels_prev", labels_prev, np.int32)
    gn, gl = b.out("centers_new", np.float32, k * d), b.out("labels", np.int32, n)
    gch, gst = b.out("changed", np.int32, 1), b.out("shift_total", np.float64, 1)
    sc = b.scratch(_scratch_bytes(n, d, k))
    code = lib.pope_kmeans_lloyd_step(gx.ptr, n, d, gc.ptr, k, gn.ptr, gl.ptr, gp.ptr, gch.ptr, gst.ptr, sc.ptr, sc.n - short,
                                      engine._stream())
    return code, b


@functools.lru_cache(maxsize=None)
def _lloyd_first_call(dev, n, d, k, skew, family, planted):
    """The first iteration (labels_prev = -1) of a case, run once and shared; verified bands, outputs as read-only arrays."""
    from graphpope_amd import engine
    x, c, far = _lloyd_input(n, d, k, family, planted)
    code, b = _lloyd_call(dev, x, c, np.full(n, -1, np.int32), skew)
    engine.check(code)
    got = b.verify()
    for v in got.values():
        v.setflags(write=False)
    return got


@pytest.mark.parametrize("family", list(LLOYD_FAMILIES))
@pytest.mark.parametrize("n,d,k,skew", LLOYD_CASES)
def test_assignment_is_the_float64_argmin(n, d, k, skew, family, dev):
    """labels against the float64 argmin of |c|^2 - 2 x.c.  A row is ambiguous when another centre's float64 score lies within
    the two float32 error bounds of the best one; on every other row the label must equal the float64 argmin exactly, on an
    ambiguous row it must be one of the centres inside that band.  The input is fit when at most 5 % of its rows are ambiguous
    (decided before the kernel's labels are looked at)."""
    best, band, ambiguous = _assign_reference(n, d, k, family)
    share = float(ambiguous.mean())
    print(f"\n[assign {n}x{d}x{k} skew={skew} {family}] ambiguous rows: {int(ambiguous.sum())} = {share:.4f} (cap {AMBIGUOUS_CAP})")
    if share > AMBIGUOUS_CAP:
        raise UnfitInput(f"{share:.3f} of the rows are ambiguous")
    labels = _lloyd_first_call(dev, n, d, k, skew, family, False)["labels"]
    assert labels.min() >= 0 and labels.max() < k
    sure = ~ambiguous
    wrong = np.nonzero(labels[sure] != best[sure])[0]
    assert wrong.size == 0, f"{wrong.size} unambiguous rows mislabelled, first: row {np.nonzero(sure)[0][wrong[:5]]}"
    assert band[np.arange(n), labels].all()


def test_assignment_ties_go_to_the_first_centre(dev):
    """K = 260 (three column tiles), D = 128: centre 5 is copied into rows 133 and 259 (another tile each), centre 130 into row
    131 (same tile, same wave).  A copy computes a bit-identical score (same depth order, same |c|^2), so the packed key's index
    half decides, inside a tile and through the atomicMin across tiles: the first wins, as argmin.  40 rows of X sit on the
    duplicated centres (+ noise of 1e-3, far below the spacing of randn centres in 128 dimensions); no row at all may get
    133, 259 or 131."""
    from graphpope_amd import engine
    n, d, k = 300, 128, 260
    rs = np.random.RandomState(n + d + k)
    c = rs.randn(k, d).astype(np.float32)
    c[133] = c[259] = c[5]
    c[131] = c[130]
    x = rs.randn(n, d).astype(np.float32)
    on = rs.permutation(n)[:40]
    target = np.where(np.arange(40) % 2 == 0, 5, 130)
    x[on] = c[target] + np.float32(1e-3) * rs.randn(40, d).astype(np.float32)
    code, b = _lloyd_call(dev, x, c, np.full(n, -1, np.int32))
    engine.check(code)
    labels = b.verify()["labels"]
    assert np.array_equal(labels[on], target)
    assert not np.isin(labels, [133, 259, 131]).any()
    s = (c.astype(np.float64) ** 2).sum(1)[None, :] - 2.0 * (x.astype(np.float64) @ c.astype(np.float64).T)
    dup = {133: 5, 259: 5, 131: 130}
    first = np.array([dup.get(int(j), int(j)) for j in s.argmin(1)])
    print(f"\n[ties] rows whose float64 argmin is a duplicated centre: {int(np.isin(first, [5, 130]).sum())} of {n}")
    assert np.array_equal(labels[on], first[on])


@pytest.mark.parametrize("family", list(LLOYD_FAMILIES))
@pytest.mark.parametrize("n,d,k,skew", LLOYD_CASES)
def test_update_is_the_float64_mean_of_the_kernels_own_labels(n, d, k, skew, family, dev):
    """centers_new / shift_total, judged against the labels the same call returned (independent of the assignment test).

    centers_new[k] = float32(float64 mean of the rows labelled k): the kernel sums in float64 in its own order, so it may differ
    from NumPy's float64 mean by N * 2^-52 * max|X| at most, and then rounds once: one float32 ulp of the expected value on top.
    Up to two planted centres at 1e6 (every shape with K >= 3 has two, K = 2 has one, K = 1 none) attract nothing: their rows
    must come back bit-identical and add exactly 0 to shift_total -- the float64 restatement of shift_total below, taken from
    the kernel's own centers_new, has exact zeros there.  shift_total: K * D float64 terms in any order, K * D * 2^-52 relative."""
    x, c, far = _lloyd_input(n, d, k, family, True)
    got = _lloyd_first_call(dev, n, d, k, skew, family, True)
    labels, new = got["labels"], got["centers_new"].reshape(k, d)
    assert labels.min() >= 0 and labels.max() < k
    counts = np.bincount(labels, minlength=k)
    assert all(counts[j] == 0 for j in far)
    x64 = x.astype(np.float64)
    sums = np.zeros((k, d))
    np.add.at(sums, labels, x64)
    filled = counts > 0
    want = c.copy()
    want[filled] = (sums[filled] / counts[filled, None]).astype(np.float32)
    tol = np.spacing(np.abs(want)).astype(np.float64) + n * 2.0 ** -52 * float(np.abs(x).max())
    err = np.abs(new.astype(np.float64) - want.astype(np.float64))
    print(f"\n[update {n}x{d}x{k} skew={skew} {family}] empty clusters {int((~filled).sum())}, worst err/tol {np.max(err[filled] / tol[filled]):.3g} (cap 1)")
    assert (err[filled] <= tol[filled]).all()
    assert np.array_equal(new[~filled].view(np.uint32), c[~filled].view(np.uint32))       # an empty cluster keeps its centre
    diff2 = (new.astype(np.float64) - c.astype(np.float64)) ** 2
    assert (diff2[~filled] == 0.0).all()
    total = float(diff2.sum())
    assert abs(float(got["shift_total"][0]) - total) <= k * d * 2.0 ** -52 * total


def test_shift_total_is_exactly_zero_when_nothing_moves(dev):
    """Every row of X is the same float32 point p; the centres are p and two far ones.  n * p is exact in float64, so the mean is
    p, the far centres are empty and keep their rows: shift_total must be exactly 0.0 (its sentinel is a NaN)."""
    from graphpope_amd import engine
    n, d = 130, 70
    p = np.random.RandomState(n + d).randn(d).astype(np.float32)
    c = np.stack([np.full(d, 1e6, np.float32), p, np.full(d, 1e6, np.float32)])
    code, b = _lloyd_call(dev, np.tile(p, (n, 1)), c, np.full(n, -1, np.int32))
    engine.check(code)
    got = b.verify()
    assert (got["labels"] == 1).all()
    assert np.array_equal(got["centers_new"].view(np.uint32), c.reshape(-1).view(np.uint32))
    assert got["shift_total"][0] == 0.0


@pytest.mark.parametrize("n,d,k,skew", LLOYD_CASES)
def test_changed_flag(n, d, k, skew, dev):
    """changed = 1 after the first call (labels_prev = -1); 0 after a call that is given those labels, which it must reproduce;
    1 again when only the last, or only the first, element of labels_prev differs."""
    from graphpope_amd import engine
    x, c, _ = _lloyd_input(n, d, k, "randn", True)
    first = _lloyd_first_call(dev, n, d, k, skew, "randn", True)
    assert first["changed"][0] == 1
    labels = first["labels"]

    def again(prev):
        code, b = _lloyd_call(dev, x, c, prev, skew)
        engine.check(code)
        return b.verify()
    second = again(labels)
    assert second["changed"][0] == 0
    assert np.array_equal(second["labels"], labels)
    assert np.array_equal(second["centers_new"].view(np.uint32), first["centers_new"].view(np.uint32))
    for pos in (n - 1, 0):
        prev = labels.copy()
        prev[pos] = labels[pos] + 1                                  # any other value; need not be a valid label
        third = again(prev)
        assert third["changed"][0] == 1, f"a change at element {pos} alone went unnoticed"
        assert np.array_equal(third["labels"], labels)


@pytest.mark.parametrize("n,d,k", [(333, 64, 129), (1, 1, 1)])
def test_one_byte_short_of_the_workspace_is_refused(n, d, k, dev):
    """scratch_bytes one below pope_kmeans_scratch_bytes: ERR_WORKSPACE, nothing launched -- every output still holds its sentinel."""
    binding, lib = _lib()
    x, c, _ = _lloyd_input(n, d, k, "randn", False)
    code, b = _lloyd_call(dev, x, c, np.full(n, -1, np.int32), short=1)
    assert code == binding.ERR_WORKSPACE
    assert b"scratch" in lib.pope_last_error()
    torch.cuda.synchronize()
    assert b.outputs_untouched() and b.all["scratch"].untouched()


# ---------------------------------------------------------------------------------------------------------------------
# 4. pope_kmeans_plusplus
# ---------------------------------------------------------------------------------------------------------------------
MARGIN_CAP = 1e-9


def _plusplus_reference(x, k, first, uniforms):
    """scikit-learn's _kmeans_plusplus with the kernel's stated roundings: squared distances summed in float64 and rounded to
    float32, `closest` the running minimum, cumulative sum and potentials in float64, cand = min(searchsorted(cum, u * pot,
    'left'), N - 1), the winner the first minimum of the candidate potentials.  Returns the chosen rows and the two smallest
    margins met on the way: min |cum[i] - u * pot| / pot, and the relative gap between the two smallest distinct candidate
    potentials (infinity when every candidate gives the same one)."""
    n = x.shape[0]
    x64 = x.astype(np.float64)

    def dist(row):
        return ((x64 - x64[row]) ** 2).sum(1).astype(np.float32)
    closest = dist(first)
    pot = float(closest.astype(np.float64).sum())
    chosen, m_cum, m_pot = [int(first)], np.inf, np.inf
    for step in range(1, k):
        cum = np.cumsum(closest.astype(np.float64))
        v = uniforms[step - 1] * pot
        cand = np.minimum(np.searchsorted(cum, v, side="left"), n - 1)
        m_cum = min(m_cum, float(np.abs(cum[None, :] - v[:, None]).min() / pot))
        newdist = np.stack([np.minimum(closest, dist(r)) for r in cand])
        pots = newdist.astype(np.float64).sum(1)
        distinct = np.unique(pots)
        if distinct.size > 1:
            m_pot = min(m_pot, float((distinct[1] - distinct[0]) / distinct[1]))
        best = int(np.argmin(pots))
        closest, pot = newdist[best], float(pots[best])
        chosen.append(int(cand[best]))
    return np.array(chosen, dtype=np.int64), m_cum, m_pot


def _plusplus_input(n, d, k, trials, blobs):
    rs = np.random.RandomState(n + d)
    if blobs:
        means = rs.randn(k, d) * 8.0
        x = means[rs.randint(0, k, n)] + rs.randn(n, d)
    else:
        x = rs.randn(n, d)
    x = x.astype(np.float32)
    x = (x - x.astype(np.float64).mean(0)).astype(np.float32)       # centred on its column means, as KMeans.fit does
    first = int(rs.randint(n))
    uniforms = np.ascontiguousarray(rs.uniform(size=(max(k - 1, 0), trials)))
    return x, first, uniforms


def _plusplus_check(dev, n, d, k, trials, blobs):
    from graphpope_amd import engine
    binding, lib = _lib()
    x, first, uniforms = _plusplus_input(n, d, k, trials, blobs)
    want, m_cum, m_pot = _plusplus_reference(x, k, first, uniforms)
    print(f"\n[k-means++ {n}x{d}x{k} trials={trials}] smallest margins: cumulative sum {m_cum:.3g}, potentials {m_pot:.3g} (both must exceed {MARGIN_CAP})")
    if not (m_cum > MARGIN_CAP and m_pot > MARGIN_CAP):
        raise UnfitInput(f"margins {m_cum:.3g} / {m_pot:.3g}: a rounding difference could flip a step")
    b = Bands(dev)
    gx = b.inp("X", x, np.float32)
    gch = b.out("chosen", np.int64, k)
    sc = b.scratch(_scratch_bytes(n, d, k))
    u_ptr = ctypes.c_void_p(uniforms.ctypes.data) if k > 1 else ctypes.c_void_p(0)      # K = 1 draws nothing: null is allowed
    engine.check(lib.pope_kmeans_plusplus(gx.ptr, n, d, k, first, u_ptr, trials, gch.ptr, sc.ptr, sc.n, engine._stream()))
    got = b.verify()["chosen"]
    assert got.dtype == np.int64 and np.array_equal(got, want), f"first difference at step {int(np.nonzero(got != want)[0][0])}"
    return got


@pytest.mark.parametrize("n,d,k,blobs", [(700, 128, 40, False), (301, 130, 17, False), (97, 3, 97, False), (1000, 16, 64, True),
                                         (513, 65, 1, False), (64, 200, 9, False)])
def test_plusplus_chooses_the_rows_of_the_numpy_restatement(n, d, k, blobs, dev):
    """`chosen`, as int64 and in order, against the restatement, with scikit-learn's trials = 2 + int(log K).  Exact because both
    margins of the input exceed 1e-9: the kernel's differently ordered float64 sums differ by ~1e-16 relative and a rare
    float32 ulp in one distance moves a cumulative sum by < 6e-8 / N relative, neither can flip a searchsorted or an argmin."""
    got = _plusplus_check(dev, n, d, k, 2 + int(np.log(k)), blobs)
    if k == n:
        assert sorted(got.tolist()) == list(range(n))               # every point is chosen exactly once


def test_plusplus_with_the_most_trials(dev):
    """n_trials = 16, the cap of the candidates' register array and of the control block."""
    _plusplus_check(dev, 301, 130, 17, 16, False)


def test_plusplus_one_byte_short_of_the_workspace_is_refused(dev):
    binding, lib = _lib()
    from graphpope_amd import engine
    n, d, k, trials = 64, 200, 9, 4
    x, first, uniforms = _plusplus_input(n, d, k, trials, False)
    b = Bands(dev)
    gx, gch = b.inp("X", x, np.float32), b.out("chosen", np.int64, k)
    sc = b.scratch(_scratch_bytes(n, d, k))
    code = lib.pope_kmeans_plusplus(gx.ptr, n, d, k, first, ctypes.c_void_p(uniforms.ctypes.data), trials, gch.ptr, sc.ptr, sc.n - 1,
                                    engine._stream())
    assert code == binding.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert b.outputs_untouched() and sc.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# 5. end to end at the depths nobody ran
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k", [(2000, 128, 20), (1500, 130, 12), (900, 65, 130)])
def test_kmeans_centers_against_scikit_learn_at_depth(n, d, k, dev):
    """engine.kmeans_centers against KMeans(n_clusters=k) from the same np.random.seed on blobs of spread 12, at the workload's
    depth (128: two full slices), a depth that is no multiple of 4 (130: generic loads, two slices and a tail of 2) and one
    past a slice with two column tiles (65, K = 130): tolerance 2e-5 * max|want|, as the test at depth 32 in
    tests/test_pairwise_gpu.py; the global NumPy stream ends where scikit-learn leaves it."""
    from sklearn.cluster import KMeans
    from graphpope_amd import engine
    rs = np.random.RandomState(n + d + k)
    means = rs.randn(k, d).astype(np.float32) * 12.0
    x = (means[rs.randint(0, k, n)] + rs.randn(n, d).astype(np.float32)).astype(np.float32)
    np.random.seed(123)
    want = KMeans(n_clusters=k).fit(x).cluster_centers_
    after_sklearn = np.random.random_sample()
    np.random.seed(123)
    got = engine.kmeans_centers(torch.as_tensor(x, device=dev), k).cpu().numpy()
    after_ours = np.random.random_sample()
    assert after_ours == after_sklearn
    assert got.shape == want.shape and got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-5 * float(np.abs(want).max()))
