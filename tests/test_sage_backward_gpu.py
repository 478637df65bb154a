"""sage_conv_backward / sage_conv_backward_indexed (and, for device extents, the two forward calls) on every kernel path, called through
the C ABI with buffers the test owns, against float64 NumPy (tests/sage_backward_cases.py: the shapes, the inputs, the reference).

Every case first asserts the path: sage_backward_kernel_name, the launch code's own plan printed, must name the kernels the shape was
picked for.  Exact family: integer inputs whose every partial sum float32 represents, compared with np.array_equal -- one lost, doubled or
stale term is a failure, whatever its size.  Rounding family: real-valued inputs within a derived bound (Reference.bounds).  Extents: the
buffers have the capacity, `dims` holds the true sizes, everything past them is poison (NaN rows, indices at NaN rows) on the input side
and a sentinel on the output side; a case's runs share their buffers, scratch included, the larger true size first."""
import ctypes

import numpy as np
import pytest
import torch

import misaligned
import sage_backward_cases as cases
from sage_backward_cases import SENTINEL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


@pytest.fixture(scope="module")
def lib():
    from graphpope_amd import _lib
    return _lib.load()


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _backward_name(lib, case, dev):
    from graphpope_amd import _lib
    n_dst = case["shape"][0]
    buf = ctypes.create_string_buffer(256)
    _lib.check(lib.sage_backward_kernel_name(n_dst, n_dst + case["extra"], case["shape"][1], case["shape"][2], int(case["grad_x"]),
                                             int(case["grad_b"]), _cus(dev), buf, 256))
    return buf.value.decode()


class Buffers:
    """Device buffers of one case at its capacities; load() fills them for a run with n true rows.  `offsets`: {attribute name: element
    offset} for the float operands to put at an address that is not 16-byte aligned (misaligned.place: self.placed lists them)."""

    def __init__(self, case, dev, nnz_cap, offsets=None):
        self.case, self.dev = case, dev
        n, c_in, c_out = case["shape"]
        self.n_cap, self.n_src_cap, self.nnz_cap = n, n + case["extra"], nnz_cap
        self.c_in, self.c_out = c_in, c_out
        offsets, self.placed = dict(offsets or {}), {}

        def alloc(name, *shape):
            if name not in offsets:
                return torch.empty(*shape, device=dev)
            self.placed[name] = misaligned.empty(shape, dev, offsets.pop(name))
            return self.placed[name]
        self.g, self.agg, self.w_l, self.w_r = alloc("g", n, c_out), alloc("agg", n, c_in), alloc("w_l", c_out, c_in), alloc("w_r", c_out, c_in)
        self.rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        self.col = torch.empty(max(nnz_cap, 1), dtype=torch.int32, device=dev)
        self.dims = torch.zeros(4, dtype=torch.int32, device=dev)
        if case["indexed"]:
            self.n_rows = self.n_src_cap + 500
            self.x = alloc("x", self.n_rows, c_in)                   # the resident feature matrix
            self.n_id = torch.empty(self.n_src_cap, dtype=torch.int64, device=dev)
        else:
            self.x = alloc("x", self.n_src_cap, c_in)
        self.grad_x = alloc("grad_x", self.n_src_cap, c_in) if case["grad_x"] else None
        self.grad_w_l, self.grad_w_r = alloc("grad_w_l", c_out, c_in), alloc("grad_w_r", c_out, c_in)
        self.grad_b = alloc("grad_b", c_out) if case["grad_b"] else None
        assert not offsets, "no such operand: %s" % sorted(offsets)
        from graphpope_amd import _lib
        lib = _lib.load()
        query = lib.sage_conv_backward_indexed_scratch_bytes if case["indexed"] else lib.sage_conv_scratch_bytes
        self.scratch_bytes = query(self.n_src_cap, n, nnz_cap, c_in, c_out)
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=dev)

    def load(self, ref, extents):
        n, n_src = ref.n, ref.n_src
        rs = np.random.RandomState(n)

        rows = lambda a, total: torch.from_numpy(cases.nan_padded(a, total))
        self.g.copy_(rows(ref.g, self.n_cap))
        self.agg.copy_(rows(ref.agg, self.n_cap))
        self.w_l.copy_(torch.from_numpy(ref.w_l))
        self.w_r.copy_(torch.from_numpy(ref.w_r))
        # entries of col past nnz point at rows of grad_x past the true sources: a scatter through them would break the sentinel there
        rowptr, col = cases.padded_csr(ref.rowptr, ref.col, self.n_cap, self.nnz_cap, n_src, self.n_src_cap, rs)
        self.rowptr.copy_(torch.from_numpy(rowptr))
        self.col.copy_(torch.from_numpy(col))
        if self.case["indexed"]:                                     # only the true destinations' rows of the matrix are numbers
            feats, n_id = cases.indexed_rows(ref.x, self.n_rows, self.n_src_cap, self.c_in, rs)
            self.x.copy_(torch.from_numpy(feats))
            self.n_id.copy_(torch.from_numpy(n_id))
        else:
            self.x.copy_(rows(ref.x, self.n_src_cap))                # (the backward pass reads the destination rows only)
        self.dims.copy_(torch.tensor([n, n_src, ref.nnz, 0], dtype=torch.int32))
        for out in (self.grad_x, self.grad_w_l, self.grad_w_r, self.grad_b):
            if out is not None:
                out.fill_(SENTINEL)
        self.extents = extents

    def run(self, lib):
        from graphpope_amd import _lib
        p = _lib.ptr
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        dims = p(self.dims) if self.extents else None
        # host-sized runs pass the true nnz; extent runs the capacity
        nnz = self.nnz_cap if self.extents else int(self.dims[2])
        if self.case["indexed"]:
            _lib.check(lib.sage_conv_backward_indexed(p(self.rowptr), p(self.col), p(self.n_id), self.n_src_cap, self.n_cap, nnz, p(self.x),
                                                      self.n_rows, p(self.agg), self.c_in, p(self.w_l), p(self.w_r), self.c_out, p(self.g),
                                                      p(self.grad_w_l), p(self.grad_b), p(self.grad_w_r), p(self.scratch),
                                                      self.scratch_bytes, dims, stream))
        else:
            _lib.check(lib.sage_conv_backward(p(self.rowptr), p(self.col), self.n_src_cap, self.n_cap, nnz, p(self.x), p(self.agg), self.c_in,
                                              p(self.w_l), p(self.w_r), self.c_out, p(self.g), p(self.grad_x), p(self.grad_w_l), p(self.grad_b),
                                              p(self.grad_w_r), p(self.scratch), self.scratch_bytes, dims, stream))
        torch.cuda.synchronize()
        got = dict(grad_w_l=self.grad_w_l, grad_w_r=self.grad_w_r)
        if self.grad_b is not None:
            got["grad_b"] = self.grad_b
        if self.grad_x is not None:
            got["grad_x"] = self.grad_x
        return {k: v.cpu().numpy().astype(np.float64) for k, v in got.items()}


def _check(case, ref, got, tag):
    """Exact family: the bits of the float64 sums.  Rounding family: within Reference.bounds (err / bound printed, cap 1).  Either way the
    rows of grad_x past the true sources still hold the sentinel."""
    if "grad_x" in got:
        beyond = got["grad_x"][ref.n_src:]
        assert np.array_equal(beyond, np.full_like(beyond, SENTINEL)), (tag, "grad_x rows past the true sources were written")
        got = dict(got, grad_x=got["grad_x"][:ref.n_src])
    if case["family"] == "exact":
        ref.assert_exact_family_is_exact()
        for k, v in got.items():
            bad = np.argwhere(v != ref.want[k])
            assert bad.size == 0, (tag, k, "%d elements differ, the first at %s: got %r, want %r"
                                   % (len(bad), tuple(bad[0]), v[tuple(bad[0])], ref.want[k][tuple(bad[0])]))
        return
    bounds = ref.bounds()
    worst = {}
    for k, v in got.items():
        assert np.isfinite(v).all(), (tag, k)
        err = np.abs(v - ref.want[k])
        worst[k] = float((err / np.maximum(bounds[k], 1e-300)).max()) if err.max() > 0 else 0.0
    print("err/bound %s %s: %s" % (case["id"], tag, ", ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, (tag, worst)


def _run_case(case, dev, lib):
    from graphpope_amd import _lib
    cap = case["shape"][0]
    lib.pope_debug_set(_lib.KNOB_STREAMK_XCD, 1 if case["xcd"] else 0)
    try:
        assert _backward_name(lib, case, dev) == cases.expected_name(case["shape"], case["extra"], case["grad_x"], case["grad_b"], case["xcd"])
        trues = case["trues"] or (cap,)
        refs = [cases.reference(case, n) for n in trues]
        buffers = Buffers(case, dev, max(r.nnz for r in refs) + (64 if case["trues"] else 0))
        for ref in refs:
            buffers.load(ref, extents=case["trues"] is not None)
            _check(case, ref, buffers.run(lib), "true %d of %d" % (ref.n, cap))
    finally:
        lib.pope_debug_set(_lib.KNOB_STREAMK_XCD, 1)


def _ids(table):
    return [c["id"] for c in table]


@pytest.mark.parametrize("case", cases.HOST_CASES, ids=_ids(cases.HOST_CASES))
def test_backward_is_exact_on_every_path(case, dev, lib):
    """Host-sized calls: every gradient equals the exact sums bit for bit, on the stream-K pair (both deals, tiles_m 1 .. 5, operand tails),
    k_gemm_dual, the split-K twin in its three tiles and both layout families, with and without rows to zero, edges, the optional
    gradients, and through the index."""
    _run_case(case, dev, lib)


def _smallest_host_case(path):
    """The smallest case of HOST_CASES on `path` with both optional gradients (and edges, without the index)."""
    table = [c for c in cases.HOST_CASES
             if cases.PATHS[c["shape"]][0] == path and c["grad_x"] and c["grad_b"] and c["edges"] and c["xcd"] and not c["indexed"]]
    return min(table, key=lambda c: (int(np.prod(c["shape"])), c["extra"]))


@pytest.mark.parametrize("path", ["dual", "twin"])
def test_backward_places_its_scratch_regions_by_the_sizes_alone(path, dev, lib):
    """sage_conv_backward with a scratch buffer of exactly sage_conv_scratch_bytes and with one 64 KiB longer: every gradient has the same
    bits in both calls and equals the reference, and the 64 KiB the library did not ask for still hold their sentinel -- the partial
    column sums of the bias gradient lie at the end of the library's own layout, not at the end of whatever buffer it was handed."""
    case = _smallest_host_case(path)
    assert _backward_name(lib, case, dev) == cases.expected_name(case["shape"], case["extra"])
    ref = cases.reference(case, case["shape"][0])
    buffers = Buffers(case, dev, ref.nnz)
    asked, tail_bytes = buffers.scratch_bytes, 64 * 1024
    assert asked > 0 and asked % 4 == 0
    buffers.load(ref, extents=False)
    exact = buffers.run(lib)
    _check(case, ref, exact, "scratch as asked")
    buffers.scratch = torch.empty(asked + tail_bytes, dtype=torch.uint8, device=dev)
    buffers.scratch_bytes = asked + tail_bytes
    tail = buffers.scratch[asked:].view(torch.float32)
    tail.fill_(SENTINEL)
    buffers.load(ref, extents=False)                                 # (the outputs hold their sentinel again)
    longer = buffers.run(lib)
    _check(case, ref, longer, "scratch 64 KiB longer")
    assert sorted(exact) == sorted(longer) == ["grad_b", "grad_w_l", "grad_w_r", "grad_x"]
    for k in exact:
        assert np.array_equal(exact[k].view(np.uint64), longer[k].view(np.uint64)), k
    assert bool((tail == SENTINEL).all()), "the bytes past sage_conv_scratch_bytes were written"


@pytest.mark.parametrize("case", cases.EXTENT_CASES, ids=_ids(cases.EXTENT_CASES))
def test_backward_with_device_extents_reads_and_writes_the_true_rows_only(case, dev, lib):
    """Capacity-sized launches with `dims`: the same exact sums over the true rows, no NaN from the poison past them, grad_x untouched past
    the true sources and holding the plain scatter sums on rows [n_dst, n_src) -- for two or three true sizes in a row on the same buffers
    and scratch, so slab or partial-sum contents of the larger run would show in the smaller one."""
    _run_case(case, dev, lib)


@pytest.mark.parametrize("case", cases.ROUNDING_CASES, ids=_ids(cases.ROUNDING_CASES))
def test_backward_rounding_stays_within_the_derived_bound(case, dev, lib):
    """Real-valued inputs, one shape per path: every element within the bound Reference.bounds derives from the number of float32 roundings
    on its way (no measured tolerance).  Worst err / bound seen on an MI355X:
    weight gradients 0.003 (515 x 37 -> 30), bias gradient below 0.001, grad_x 0.117 (1030 x 40 -> 24)."""
    _run_case(case, dev, lib)


# ---- forward, extents only (the host-sized forward paths have their tests in test_sage_gpu.py) ----
class _knob_at_zero:
    """pope_debug_set(knob, 0) for the length of a with block (knob: a name in _lib, or None)."""

    def __init__(self, lib, knob):
        from graphpope_amd import _lib
        self.lib, self.knob = lib, getattr(_lib, knob) if knob else None

    def __enter__(self):
        if self.knob is not None:
            self.lib.pope_debug_set(self.knob, 0)

    def __exit__(self, *exc):
        if self.knob is not None:
            self.lib.pope_debug_set(self.knob, 1)
        return False


@pytest.mark.parametrize("indexed", [False, True], ids=["plain", "indexed"])
@pytest.mark.parametrize("shape,knob,name", cases.FORWARD,
                         ids=["%dx%d-%d%s" % (s + ("" if k is None else "-" + k[5:].lower() + "0",)) for s, k, _ in cases.FORWARD])
def test_forward_with_device_extents_reads_and_writes_the_true_rows_only(shape, knob, name, indexed, dev, lib):
    """sage_conv_forward / sage_conv_forward_indexed at a capacity with `dims`, in each of the four forms of the projection: `agg`, `out`
    (and x_dst) are exact on the true rows (cases.ForwardReference: integer inputs) and keep their sentinel beyond; the NaN rows past the
    true sources and the indices that point at them leave no trace.  Two true sizes in a row on the same buffers, the larger first."""
    from graphpope_amd import _lib
    p = _lib.ptr
    cap, c_in, c_out = shape
    n_src_cap, n_rows = cap + cases.FORWARD_EXTRA, cap + cases.FORWARD_EXTRA + 500
    buf = ctypes.create_string_buffer(96)
    with _knob_at_zero(lib, knob):
        _lib.check(lib.sage_forward_kernel_name(cap, c_in, c_out, _cus(dev), buf, 96))
    assert buf.value.decode() == name
    refs = [cases.forward_reference(n, c_in, c_out) for n in cases.forward_trues(cap)]
    nnz_cap = max(r.nnz for r in refs) + 64
    f = lambda *s: torch.empty(*s, device=dev)
    x_d, col_d = f(n_rows if indexed else n_src_cap, c_in), torch.empty(nnz_cap, dtype=torch.int32, device=dev)
    agg_d, out_d, xdst_d = f(cap, c_in), f(cap, c_out), f(cap, c_in)
    sbytes = (lib.sage_conv_forward_indexed_scratch_bytes if indexed else lib.sage_conv_forward_scratch_bytes)(cap, c_in, c_out)
    scratch = torch.empty(max(sbytes, 16), dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ref in refs:
        n, rs = ref.n, np.random.RandomState(ref.n)
        ref.assert_exact_family_is_exact()
        rowptr, col = cases.padded_csr(ref.rowptr, ref.col, cap, nnz_cap, ref.n_src, n_src_cap, rs)    # past nnz: sources that are NaN rows
        if indexed:
            feats, n_id = cases.indexed_rows(ref.x, n_rows, n_src_cap, c_in, rs)
            nid_d = torch.from_numpy(n_id).to(dev)
        else:
            feats = cases.nan_padded(ref.x, n_src_cap)
        x_d.copy_(torch.from_numpy(feats))
        col_d.copy_(torch.from_numpy(col))
        rp_d, wl_d, wr_d, b_d = (torch.from_numpy(a).to(dev) for a in (rowptr, ref.w_l, ref.w_r, ref.b))
        dims = torch.tensor([n, ref.n_src, ref.nnz, 0], dtype=torch.int32, device=dev)
        for t in (agg_d, out_d, xdst_d):
            t.fill_(SENTINEL)
        with _knob_at_zero(lib, knob):
            if indexed:
                _lib.check(lib.sage_conv_forward_indexed(p(rp_d), p(col_d), p(nid_d), n_src_cap, cap, nnz_cap, p(x_d), n_rows, c_in, p(wl_d),
                                                         p(b_d), p(wr_d), c_out, p(agg_d), p(xdst_d), p(out_d), p(scratch), sbytes, p(dims), stream))
            else:
                _lib.check(lib.sage_conv_forward(p(rp_d), p(col_d), n_src_cap, cap, nnz_cap, p(x_d), c_in, p(wl_d), p(b_d), p(wr_d), c_out,
                                                 p(agg_d), p(out_d), p(scratch), sbytes, p(dims), stream))
            torch.cuda.synchronize()
        want = [("agg", agg_d, ref.agg), ("out", out_d, ref.out)] + ([("x_dst", xdst_d, ref.x[:n].astype(np.float64))] if indexed else [])
        for what, got_d, w in want:
            got = got_d.cpu().numpy().astype(np.float64)
            assert np.array_equal(got[:n], w), (n, what, int((got[:n] != w).sum()))
            assert np.array_equal(got[n:], np.full_like(got[n:], SENTINEL)), (n, what, "rows past the true count were written")
