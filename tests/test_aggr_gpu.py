"""The two halves of SAGEConv(aggr='add' | 'max') on the GPU -- sage_aggregate_forward (k_gather_reduce) and sage_aggregate_backward (the
index build and k_scatter_ordered) -- held bit for bit to the sequential restatement of tests/aggr_cases.py: every degree remainder of
the four-in-flight loop, a row past a 64-lane chunk, repeated neighbours, a hub whose list is longer than a wave, scalar and vector
widths with a second slab and a tail, ties, a negative column, a NaN, sources nobody lists, operands off their 16-byte alignment,
indexed mode, device extents below the capacities, a poisoned and guard-banded scratch, arg = NULL, and two calls for equal bits."""
import ctypes

import numpy as np
import pytest
import torch

import aggr_cases as cases
from workspace import FILLS, GuardedScratch, dev, lib  # noqa: F401  (the fixtures live in the helper module)

pytestmark = pytest.mark.gpu

WIDTHS = (1, 13, 64, 260)            # scalar; scalar with a remainder; one vector slab; two slabs with a tail (260 = 256 + 4)


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    """A fault is sticky: every later call in the process would fail the same way.  The run ends at the test that met it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the GPU reported an error, nothing more is started: %s" % e, returncode=3)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(0) if t is None else ctypes.c_void_p(t.data_ptr())


def _put(dev, a, shift=0, room=0, fill=0):
    """`a` on the device, `shift` elements into an allocation of its own (shift = 1: off the 16-byte alignment), with `room` more elements
    behind it holding `fill`."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a).reshape(-1)
    buf = torch.full((shift + t.numel() + room,), fill, dtype=t.dtype, device=dev)
    buf[shift:shift + t.numel()] = t.to(dev)
    view = buf[shift:]
    assert view.data_ptr() % 16 == (4 * shift) % 16 or t.element_size() != 4
    return view


def same_bits(a, b):
    """Equal bits, a NaN standing for any NaN (an addition may quieten or re-sign one; a maximum copies it)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def forward(lib, dev, rowptr, col, x, aggr, n_id=None, want_arg=True, shift=0, caps=None, dims=None, x_dst=False):
    """sage_aggregate_forward over host arrays: (agg, arg, x_dst) as NumPy, at the capacities `caps` = (n_dst, n_src, nnz) if given (the
    outputs are then pre-filled with a pattern; `dims`: the true sizes, on the device)."""
    from graphpope_amd import _lib
    n_dst, nnz = len(rowptr) - 1, len(col)
    n_src = len(n_id) if n_id is not None else x.shape[0]
    if caps:
        n_dst, n_src, nnz = caps
    c = x.shape[1]
    d_rowptr, d_col, d_x = _put(dev, rowptr.astype(np.int32), shift), _put(dev, col.astype(np.int32), shift), _put(dev, x, shift)
    d_nid = None if n_id is None else _put(dev, n_id.astype(np.int64))
    agg = _put(dev, np.full((n_dst, c), 7.5, np.float32), shift)
    arg = _put(dev, np.full((n_dst, c), -77, np.int32), shift) if want_arg and aggr == "max" else None
    xd = _put(dev, np.full((n_dst, c), 7.5, np.float32), shift) if x_dst else None
    d_dims = None if dims is None else torch.tensor(list(dims) + [0], dtype=torch.int32, device=dev)
    _lib.check(lib.sage_aggregate_forward(_p(d_rowptr), _p(d_col), _p(d_nid), n_src, n_dst, nnz, _p(d_x), x.shape[0], c, cases.AGGR_ID[aggr],
                                          _p(agg), _p(arg), _p(xd), _p(d_dims), _stream()))
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t[:n_dst * c].cpu().numpy().reshape(n_dst, c)
    return host(agg), host(arg), host(xd)


def backward(lib, dev, rowptr, col, n_src, n_dst, grad_agg, grad_x, aggr, arg=None, shift=0, caps=None, dims=None, scratch=None, refuse=False):
    """sage_aggregate_backward over host arrays: the grad_x left behind (all the rows given).  scratch: a GuardedScratch, else a fresh
    buffer of the queried size (shift: 4 bytes into its allocation)."""
    from graphpope_amd import _lib
    nnz = len(col)
    if caps:
        n_dst, n_src, nnz = caps
    c = grad_agg.shape[1]
    d_rowptr, d_col = _put(dev, rowptr.astype(np.int32), shift), _put(dev, col.astype(np.int32), shift)
    d_gagg, d_gx = _put(dev, grad_agg, shift), _put(dev, grad_x, shift)
    d_arg = None if arg is None else _put(dev, arg.astype(np.int32), shift)
    d_dims = None if dims is None else torch.tensor(list(dims) + [0], dtype=torch.int32, device=dev)
    need = lib.sage_aggregate_backward_scratch_size(n_src, n_dst, nnz)
    if scratch is None:
        buf = torch.empty(need + 16, dtype=torch.uint8, device=dev)
        s_ptr, s_bytes = ctypes.c_void_p(buf.data_ptr() + 4 * shift), need
    else:
        s_ptr, s_bytes = scratch.short() if refuse else (scratch.ptr, scratch.nbytes)
    rc = lib.sage_aggregate_backward(_p(d_rowptr), _p(d_col), n_src, n_dst, nnz, _p(d_arg), _p(d_gagg), c, cases.AGGR_ID[aggr], _p(d_gx), s_ptr,
                                     s_bytes, _p(d_dims), _stream())
    torch.cuda.synchronize()
    if refuse:
        return rc, d_gx[:grad_x.size].cpu().numpy().reshape(grad_x.shape)
    _lib.check(rc)
    return d_gx[:grad_x.size].cpu().numpy().reshape(grad_x.shape)


def _grads(n_dst, rows, c, seed):
    """(grad_agg [n_dst, c], the grad_x found on entry [rows, c] with a -0.0 and exact zeros among its values)."""
    rs = np.random.RandomState(seed)
    g = rs.standard_normal((n_dst, c)).astype(np.float32)
    into = rs.standard_normal((rows, c)).astype(np.float32)
    into[rs.random_sample((rows, c)) < 0.2] = 0.0
    into[0, 0] = -0.0
    return g, into


# ------------------------------------------------------------------------------------------------ degrees, widths, values

@pytest.mark.parametrize("square", [False, True], ids=["n_dst<n_src", "n_dst=n_src"])
@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_both_halves_equal_the_restatement_bit_for_bit(lib, dev, aggr, c, square):
    """Rows of degree 0, 1 .. 9, 70 and rows that repeat a neighbour; column 0 negative throughout, 60 % exact zeros elsewhere, one NaN in a
    listed source; the last three sources listed by nobody.  Forward: agg and arg; without arg the same agg; a second call the same bits.
    Backward, from a grad_x that holds values (a -0.0 among them) in its destination rows and a pattern behind them."""
    n_src = 20 if square else 40
    rowptr, col = cases.degree_block(n_src, seed=c, extra_dst=8 if square else 6)
    n_dst = len(rowptr) - 1
    assert (n_dst == n_src) == square and set(np.diff(rowptr)) >= set(range(10)) | {70}
    x = cases.half_values(n_src, c, seed=10 + c, nan_at=(int(col[rowptr[9] + 2]), c // 2))
    want_agg, want_arg = cases.gather_restate(rowptr, col, x, aggr)
    assert np.isnan(want_agg).any() and ((want_agg[1:, 0] < 0) | np.isnan(want_agg[1:, 0])).all()
    agg, arg, _ = forward(lib, dev, rowptr, col, x, aggr)
    assert same_bits(agg, want_agg)
    if aggr == "max":
        assert np.array_equal(arg, want_arg) and (arg[0] == -1).all()
        assert c == 1 or (want_agg[1:, 1:] == 0).any()              # ties were there to be broken
        agg_noarg, none, _ = forward(lib, dev, rowptr, col, x, aggr, want_arg=False)
        assert none is None and same_bits(agg_noarg, want_agg)
    again = forward(lib, dev, rowptr, col, x, aggr)
    assert same_bits(again[0], agg) and (aggr == "add" or np.array_equal(again[1], arg))

    g, into = _grads(n_dst, n_src + 2, c, seed=20 + c)
    want = cases.scatter_restate(rowptr, col, n_src, n_dst, g, into, aggr, want_arg)
    got = backward(lib, dev, rowptr, col, n_src, n_dst, g, into, aggr, want_arg)
    assert same_bits(got, want)
    assert np.array_equal(got[n_src:], into[n_src:]) and np.signbit(got[0, 0]) == np.signbit(want[0, 0])
    if not square:
        assert not got[n_src - 3:n_src].any()                       # rows behind the destinations that nobody lists: overwritten with +0
    assert same_bits(backward(lib, dev, rowptr, col, n_src, n_dst, g, into, aggr, want_arg), got)


@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_hub_source_listed_by_130_destinations(lib, dev, aggr):
    """One source in the rows of 130 destinations (twice in some): its list is longer than a wave, so it is ranked through the scratch
    buffer and summed by one wave over both slabs of c = 260."""
    n_src, c = 140, 260
    rowptr, col = cases.hub_block(n_src)
    n_dst = len(rowptr) - 1
    assert n_dst == 130 and (col == 3).sum() > 130
    x = cases.half_values(n_src, c, seed=3)
    want_agg, want_arg = cases.gather_restate(rowptr, col, x, aggr)
    agg, arg, _ = forward(lib, dev, rowptr, col, x, aggr)
    assert same_bits(agg, want_agg) and (aggr == "add" or np.array_equal(arg, want_arg))
    g, into = _grads(n_dst, n_src, c, seed=4)
    want = cases.scatter_restate(rowptr, col, n_src, n_dst, g, into, aggr, want_arg)
    got = backward(lib, dev, rowptr, col, n_src, n_dst, g, into, aggr, want_arg)
    assert same_bits(got, want)
    if aggr == "max":
        assert 0 < (want_arg == 3).sum() < want_arg.size            # the hub wins some columns and loses others
    assert same_bits(backward(lib, dev, rowptr, col, n_src, n_dst, g, into, aggr, want_arg), got)


@pytest.mark.parametrize("c", (64, 260))
@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_every_operand_offset_by_one_float(lib, dev, aggr, c):
    """rowptr, col, x, agg, arg, grad_agg, grad_x and the scratch each start four bytes into their allocation: the widths that take
    16-byte accesses fall back to scalar ones, with the same values."""
    n_src = 40
    rowptr, col = cases.degree_block(n_src, seed=7, extra_dst=6)
    n_dst = len(rowptr) - 1
    x = cases.half_values(n_src, c, seed=8)
    want_agg, want_arg = cases.gather_restate(rowptr, col, x, aggr)
    agg, arg, _ = forward(lib, dev, rowptr, col, x, aggr, shift=1)
    assert same_bits(agg, want_agg) and (aggr == "add" or np.array_equal(arg, want_arg))
    g, into = _grads(n_dst, n_src + 1, c, seed=9)
    got = backward(lib, dev, rowptr, col, n_src, n_dst, g, into, aggr, want_arg, shift=1)
    assert same_bits(got, cases.scatter_restate(rowptr, col, n_src, n_dst, g, into, aggr, want_arg))


@pytest.mark.parametrize("c", (13, 64))
@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_indexed_mode_reads_through_n_id_and_writes_x_dst(lib, dev, aggr, c):
    """n_id: a permutation into a 200-row matrix.  agg is the restatement's through n_id, arg the POSITION in n_id (not the feature row),
    x_dst the destinations' own rows."""
    n_src = 40
    rowptr, col = cases.degree_block(n_src, seed=11, extra_dst=6)
    n_dst = len(rowptr) - 1
    n_id = np.random.RandomState(3).permutation(200)[:n_src].astype(np.int64)
    feats = cases.half_values(200, c, seed=12)
    want_agg, want_arg = cases.gather_restate(rowptr, col, feats, aggr, n_id=n_id)
    agg, arg, x_dst = forward(lib, dev, rowptr, col, feats, aggr, n_id=n_id, x_dst=True)
    assert same_bits(agg, want_agg) and same_bits(x_dst, feats[n_id[:n_dst]])
    if aggr == "max":
        assert np.array_equal(arg, want_arg) and arg.max() < n_src and not np.array_equal(n_id[np.maximum(arg, 0)], np.maximum(arg, 0))
        assert same_bits(want_agg, cases.gather_restate(rowptr, col, feats[n_id], aggr)[0])


@pytest.mark.parametrize("c", (13, 64))
@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_device_extents_below_the_capacities(lib, dev, aggr, c):
    """The sizes are capacities; the true {n_dst, n_src} stand in a device word triple, and what lies behind them in rowptr and col is
    garbage that is never followed.  Every byte of the outputs outside the true extents keeps its pattern."""
    n_src = 40
    rowptr, col = cases.degree_block(n_src, seed=13, extra_dst=6)
    n_dst, nnz = len(rowptr) - 1, len(col)
    caps = (n_dst + 9, n_src + 11, nnz + 50)
    big_rowptr = np.concatenate([rowptr, np.full(9, 1 << 30, np.int32)])
    big_col = np.concatenate([col, np.full(50, 1 << 29, np.int32)])
    x = cases.half_values(caps[1], c, seed=14)
    want_agg, want_arg = cases.gather_restate(rowptr, col, x, aggr)
    agg, arg, _ = forward(lib, dev, big_rowptr, big_col, x, aggr, caps=caps, dims=(n_dst, n_src, nnz))
    assert same_bits(agg[:n_dst], want_agg) and (agg[n_dst:] == 7.5).all()
    if aggr == "max":
        assert np.array_equal(arg[:n_dst], want_arg) and (arg[n_dst:] == -77).all()
    g, into = _grads(caps[0], caps[1] + 1, c, seed=15)
    full_arg = None if aggr == "add" else np.concatenate([want_arg, np.full((9, c), 5, np.int32)])
    want = cases.scatter_restate(rowptr, col, n_src, n_dst, g[:n_dst], into, aggr, want_arg)
    got = backward(lib, dev, big_rowptr, big_col, n_src, n_dst, g, into, aggr, full_arg, caps=caps, dims=(n_dst, n_src, nnz))
    assert same_bits(got, want) and np.array_equal(got[n_src:], into[n_src:])


@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_slots_and_sources_out_of_range_are_skipped(lib, dev, aggr):
    """col entries outside [0, n_src) are skipped by both halves, never followed: the results are those of the block without them."""
    n_src, c = 40, 13
    rowptr, col = cases.degree_block(n_src, seed=17, extra_dst=6)
    n_dst = len(rowptr) - 1
    bad = col.copy()
    at = [int(rowptr[5]), int(rowptr[9] + 3), int(rowptr[10] + 65), int(rowptr[11] + 1)]
    bad[at] = [-1, n_src, 1 << 30, -(1 << 31)]
    keep = np.ones(len(col), bool)
    keep[at] = False
    clean_col = col[keep]
    clean_rowptr = np.concatenate([[0], np.cumsum([keep[rowptr[i]:rowptr[i + 1]].sum() for i in range(n_dst)])]).astype(np.int32)
    x = cases.half_values(n_src, c, seed=18)
    want_agg, want_arg = cases.gather_restate(clean_rowptr, clean_col, x, aggr)
    agg, arg, _ = forward(lib, dev, rowptr, bad, x, aggr)
    assert same_bits(agg, want_agg) and (aggr == "add" or np.array_equal(arg, want_arg))
    g, into = _grads(n_dst, n_src, c, seed=19)
    got = backward(lib, dev, rowptr, bad, n_src, n_dst, g, into, aggr, want_arg)
    assert same_bits(got, cases.scatter_restate(clean_rowptr, clean_col, n_src, n_dst, g, into, aggr, want_arg))


# ------------------------------------------------------------------------------------------------ the caller's scratch

@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_scratch_is_contained_self_initialising_and_refused_when_short(lib, dev, aggr):
    """The hub block (its long list is ranked THROUGH the scratch buffer): 4096 guard bytes on both sides stay as they were; zeros, 0xFF,
    random bytes or another call's leftovers in the buffer change no bit of the result; a buffer one byte short is POPE_ERR_WORKSPACE and
    neither it nor grad_x moves."""
    from graphpope_amd import _lib
    n_src, c = 140, 64
    rowptr, col = cases.hub_block(n_src)
    n_dst = len(rowptr) - 1
    x = cases.half_values(n_src, c, seed=5)
    _, arg = cases.gather_restate(rowptr, col, x, aggr)
    g, into = _grads(n_dst, n_src, c, seed=6)
    want = cases.scatter_restate(rowptr, col, n_src, n_dst, g, into, aggr, arg)
    scratch = GuardedScratch(dev, lib.sage_aggregate_backward_scratch_size(n_src, n_dst, len(col)))
    for fill in FILLS:
        scratch.fill(fill)
        assert same_bits(backward(lib, dev, rowptr, col, n_src, n_dst, g, into, aggr, arg, scratch=scratch), want), fill
        assert scratch.bands_intact(), fill
    scratch.fill("noise")
    before = scratch.snapshot()
    rc, untouched = backward(lib, dev, rowptr, col, n_src, n_dst, g, into, aggr, arg, scratch=scratch, refuse=True)
    assert rc == _lib.ERR_WORKSPACE and str(scratch.nbytes).encode() in lib.pope_last_error()
    assert scratch.unchanged_since(before) and np.array_equal(untouched.view(np.uint32), into.view(np.uint32))
