"""The row L2 normalisation on the GPU (sage_l2_normalize_forward / _backward, csrc/l2norm.hip), called directly through
tests/l2norm_cases.py: every shape of the table on 16-byte aligned operands and on operands 4 bytes off that grid, within the rounding
bounds against float64; the exactly stated rows; device extents; aliasing; equal bits from call to call and between the vector and the
scalar instantiation.  Every operand lies between two bands of 64 sentinel floats that must not move by a bit."""
import ctypes

import numpy as np
import pytest
import torch

import l2norm_cases as cases
from workspace import dev, lib  # noqa: F401  (the fixtures live in the helper module)

pytestmark = pytest.mark.gpu

BAND = 64
SENTINEL_BITS = 0x4640E400            # 12345.0f
POISON_BITS = 0x7FA00BAD              # a NaN with a payload: rows beyond the device extent must keep it bit for bit


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    """A fault is sticky: every later call in the process would fail the same way.  The run ends at the test that met it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the GPU reported an error, nothing more is started: %s" % e, returncode=3)


class Banded:
    """A float32 operand of `shape` at element offset BAND + off of a buffer of its own; everything around it holds the sentinel.  The
    buffer is 256-byte aligned and BAND floats are 256 bytes, so the operand is 4 * off bytes past a 16-byte boundary (asserted)."""

    def __init__(self, dev, shape, off, fill=None, bits=None):
        n = int(np.prod(shape))
        self.buf = torch.full((BAND + off + n + BAND,), SENTINEL_BITS, dtype=torch.int32, device=dev)
        assert self.buf.data_ptr() % 256 == 0
        self.lo, self.n = BAND + off, n
        self.view = self.buf[self.lo:self.lo + n].view(torch.float32).view(shape)
        assert self.view.data_ptr() % 16 == (4 * off) % 16 and self.view.is_contiguous()
        if fill is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float32)))
        elif bits is not None:
            self.buf[self.lo:self.lo + n] = bits

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def host(self):
        return self.view.cpu().numpy()

    def bands_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:self.lo] == SENTINEL_BITS).all() and (b[self.lo + self.n:] == SENTINEL_BITS).all())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(lib, dev, x, g, off=0, m=None, rows_dev=None, alias=False, out_bits=None):
    """Forward then backward over the first `m` rows (default: all) of operands placed at `off`; the three results on the host, after
    the bands of all five operands were found intact.  alias: y is x and grad_x is grad_y.  out_bits: what the outputs hold before."""
    from graphpope_amd import _lib
    rows, c = x.shape
    m = rows if m is None else m
    bx, bg = Banded(dev, (rows, c), off, fill=x), Banded(dev, (rows, c), off, fill=g)
    by = bx if alias else Banded(dev, (rows, c), off, bits=out_bits)
    bgx = bg if alias else Banded(dev, (rows, c), off, bits=out_bits)
    binv = Banded(dev, (rows,), 0, bits=out_bits)
    nothing = ctypes.c_void_p(0)
    rd = nothing if rows_dev is None else ctypes.c_void_p(rows_dev.data_ptr())
    _lib.check(lib.sage_l2_normalize_forward(bx.ptr, m, c, cases.EPS, by.ptr, binv.ptr, rd, _stream()))
    _lib.check(lib.sage_l2_normalize_backward(by.ptr, binv.ptr, bg.ptr, m, c, cases.EPS, bgx.ptr, rd, _stream()))
    torch.cuda.synchronize()
    for b in (bx, bg, by, bgx, binv):
        assert b.bands_intact()
    if not alias:
        assert np.array_equal(_bits(bx.host()), _bits(x)) and np.array_equal(_bits(bg.host()), _bits(g))          # inputs untouched
    return cases.Result(by.host(), binv.host(), bgx.host())


def _same_bits(a, b):
    return all(np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))) for k in ("y", "inv", "gx"))


def _kernel_names(lib, m, c, mask):
    from graphpope_amd import _lib
    buf = ctypes.create_string_buffer(96)
    _lib.check(lib.sage_l2_normalize_kernel_name_at(m, c, mask, buf, 96))
    return buf.value.decode()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off4bytes"])
@pytest.mark.parametrize("c", cases.CS)
def test_grid_within_the_bounds(lib, dev, c, off):
    """Every M of the table at this width.  The instantiation is the one the query names: 16-byte accesses only for C % 4 == 0 on aligned
    operands, so the two parametrisations of C in {64, 256, 300} run both.  Two calls give equal bits, and so do the two instantiations."""
    vec = "true" if (c % 4 == 0 and off == 0) else "false"
    for case in (k for k in cases.GRID if k.c == c):
        assert _kernel_names(lib, case.m, c, 0xF if off else 0) == "k_l2_normalize<%s>+k_l2_normalize_backward<%s>" % (vec, vec)
        x, g = cases.inputs(case)
        got = _run(lib, dev, x, g, off)
        print(case.id, "off", off, "worst error / bound", cases.worst_ratio(case, got))
        assert cases.violations(case, got) == {"y": 0, "inv": 0, "gx": 0}, case.id
        assert _same_bits(got, _run(lib, dev, x, g, off)), case.id
        if off:
            assert _same_bits(got, _run(lib, dev, x, g, 0)), case.id


def test_both_instantiations_are_reached(lib):
    seen = {_kernel_names(lib, k.m, k.c, mask) for k in cases.GRID for mask in (0, 0xF)}
    assert seen == {"k_l2_normalize<true>+k_l2_normalize_backward<true>", "k_l2_normalize<false>+k_l2_normalize_backward<false>"}
    assert any(k.c % 4 == 0 for k in cases.GRID) and any(k.c > 256 for k in cases.GRID)          # a second stride of the wave too


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off4bytes"])
@pytest.mark.parametrize("case", cases.SPECIAL, ids=lambda k: k.id)
def test_special_rows(lib, dev, case, off):
    """The all-zero row, the row below eps, the rows with a NaN and an inf and the row whose squares overflow give the stated values
    exactly; the random rows between them stay inside the bounds: no row touches its neighbour."""
    x, g = cases.inputs(case)
    got = _run(lib, dev, x, g, off)
    for row, want in cases.special_expectation(case).items():
        kind = cases.SPECIAL_ROWS[row]
        assert cases.same_values(got.y[row], want.y), (kind, "y", got.y[row][:8])
        assert cases.same_values(got.inv[row], want.inv), (kind, "inv_norm", got.inv[row])
        assert cases.same_values(got.gx[row], want.gx), (kind, "grad_x", got.gx[row][:8])
    print(case.id, "off", off, "worst error / bound", cases.worst_ratio(case, got))
    assert cases.violations(case, got) == {"y": 0, "inv": 0, "gx": 0}
    rest = [r for r in range(case.m) if r not in cases.SPECIAL_ROWS]
    assert np.isfinite(got.y[rest]).all() and np.isfinite(got.gx[rest]).all() and np.isfinite(got.inv[rest]).all()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off4bytes"])
@pytest.mark.parametrize("c", [7, 256])
def test_device_extent(lib, dev, c, off):
    """Buffers of 300 rows, the true count 257 in a device word: rows 257 .. of y, inv_norm and grad_x keep their poison bit for bit
    (neither read nor written: the inputs there are NaN and would show), the rows below carry the bits of the M = 257 call."""
    case = cases.Case("grid", 257, c)
    x, g = cases.inputs(case)
    cap = 300
    xx, gg = np.full((cap, c), np.nan, dtype=np.float32), np.full((cap, c), np.nan, dtype=np.float32)
    xx[:257], gg[:257] = x, g
    rows_dev = torch.tensor([257], dtype=torch.int32, device=dev)
    got = _run(lib, dev, xx, gg, off, rows_dev=rows_dev, out_bits=POISON_BITS)
    want = _run(lib, dev, x, g, off)
    assert _same_bits(cases.Result(got.y[:257], got.inv[:257], got.gx[:257]), want)
    for t in (got.y[257:], got.inv[257:], got.gx[257:]):
        assert (_bits(t) == POISON_BITS).all()
    # a count beyond the capacity is the capacity, a negative one is zero rows
    over = _run(lib, dev, x, g, off, rows_dev=torch.tensor([10 ** 6], dtype=torch.int32, device=dev))
    assert _same_bits(over, want)
    none = _run(lib, dev, x, g, off, rows_dev=torch.tensor([-5], dtype=torch.int32, device=dev), out_bits=POISON_BITS)
    assert all((_bits(t) == POISON_BITS).all() for t in (none.y, none.inv, none.gx))


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off4bytes"])
@pytest.mark.parametrize("case", [cases.Case("grid", 257, 300), cases.Case("grid", 255, 63), cases.Case("special", cases.SPECIAL_M, 64)],
                         ids=lambda k: k.id)
def test_aliased_outputs_give_the_same_bits(lib, dev, case, off):
    """y is x and grad_x is grad_y: the bits of the out-of-place calls (C = 300: rows wider than one stride of the wave)."""
    x, g = cases.inputs(case)
    assert _same_bits(_run(lib, dev, x, g, off, alias=True), _run(lib, dev, x, g, off))


def test_wide_rows_beyond_the_register_window(lib, dev):
    """C = 1 100 (vector form) and 1 101 (scalar form): more than four packs per lane, so the tail of every row is read a second time --
    in place as well.  Same reference, same bounds."""
    for c in (1100, 1101):
        rs = np.random.RandomState(c)
        x = cases._away_from_zero(rs.randn(5, c)).astype(np.float32)
        g = cases._away_from_zero(rs.randn(5, c)).astype(np.float32)
        ref, clamped, bound = cases.reference(x, g)
        got = _run(lib, dev, x, g)
        assert not clamped.any()
        for name in ("y", "inv", "gx"):
            assert (np.abs(getattr(got, name).astype(np.float64) - getattr(ref, name)) <= getattr(bound, name)).all(), (c, name)
        assert _same_bits(got, _run(lib, dev, x, g, alias=True)) and _same_bits(got, _run(lib, dev, x, g, 1))
