"""The plans' alignment inputs, without a GPU: the *_kernel_name_at queries (the launch code's own plan functions, printed) against
tests/misaligned_cases.py, the table of what a call with operands that are not 16-byte aligned must launch on 256 compute units."""
import ctypes

import numpy as np
import pytest

import misaligned_cases as cases
import pairwise_plan_cases as pw
import sage_backward_cases as bw


@pytest.fixture(scope="module")
def lib():
    from graphpope_amd import _lib
    return _lib.load()


def _name(fn, *args):
    from graphpope_amd import _lib
    buf = ctypes.create_string_buffer(384)
    _lib.check(fn(*args, buf, 384))
    return buf.value.decode()


def forward_at(lib, shape, mask):
    return _name(lib.sage_forward_kernel_name_at, *shape, cases.CUS, mask)


def backward_at(lib, shape, extra, mask, grad_x=1, grad_b=1):
    n, c_in, c_out = shape
    return _name(lib.sage_backward_kernel_name_at, n, n + extra, c_in, c_out, grad_x, grad_b, cases.CUS, mask)


def pairwise_at(lib, row, mask):
    return _name(lib.pope_pairwise_kernel_name_at, *row[:6], cases.CUS, mask)


def finalize_at(lib, has_x, mask):
    n, k, f = cases.FINALIZE_SHAPE
    return _name(lib.pope_finalize_kernel_name_at, n, k, f, has_x, 1, mask)


def test_forward_table(lib):
    seen = []
    for shape, mode, operand in cases.FORWARD_ROWS:
        mask = cases.FORWARD_OPERANDS[mode][operand]
        got = forward_at(lib, shape, mask)
        assert got == cases.forward_name(shape, mode, operand), (shape, mode, operand)
        assert (got != cases.FORWARD_ALIGNED[shape]) == (mask != 0), (shape, mode, operand)
        assert forward_at(lib, shape, 0) == _name(lib.sage_forward_kernel_name, *shape, cases.CUS) == cases.FORWARD_ALIGNED[shape]
        assert cases.FORWARD_ALIGNED[shape] in [n for s, _, n in bw.FORWARD if s == shape]       # the shapes are rows of cases.FORWARD
        seen.append(got)
    for alt in cases.ALTERNATIVES["forward"]:
        assert any(alt in s for s in seen), alt


def test_backward_table(lib):
    seen = []
    for shape, operand, extra in cases.BACKWARD_ROWS:
        mask = cases.BACKWARD_OPERANDS[operand]
        got = backward_at(lib, shape, extra, mask)
        assert got == cases.backward_name(shape, operand, extra), (shape, operand, extra)
        old = _name(lib.sage_backward_kernel_name, shape[0], shape[0] + extra, shape[1], shape[2], 1, 1, cases.CUS)
        assert backward_at(lib, shape, extra, 0) == old == bw.expected_name(shape, extra) == cases.backward_name(shape, "grad_b", extra)
        seen.append(got)
    # every flag operand but grad_x (which only the deterministic sum looks at) changes the name at every shape
    for shape in cases.BACKWARD_SHAPES:
        for operand in ("g", "agg", "x", "w_l", "w_r", "all"):
            assert cases.backward_name(shape, operand, 300) != cases.backward_name(shape, "grad_b", 300), (shape, operand)
        assert cases.backward_name(shape, "grad_x", 300) == cases.backward_name(shape, "grad_b", 300)
    for mask, want in (cases.INDEXED_ALIGNED, cases.INDEXED_X, cases.INDEXED_X_TMP):
        for extra in (0, 300):
            got = backward_at(lib, cases.INDEXED_SHAPE, extra, mask, grad_x=0)
            assert got == want, (mask, extra)
            seen.append(got)
    assert backward_at(lib, cases.INDEXED_SHAPE, 0, 0, grad_x=0) == bw.expected_name(cases.INDEXED_SHAPE, 0, grad_x=False) == cases.INDEXED_ALIGNED[1]
    from graphpope_amd import _lib
    was = lib.sage_set_deterministic(1)
    try:
        for mask, want in cases.DET_ROWS:
            got = backward_at(lib, cases.DET_SHAPE, 300, mask)
            assert got == want, mask
            seen.append(got)
        assert backward_at(lib, cases.DET_SHAPE, 300, 0) == _name(lib.sage_backward_kernel_name, 4160, 4460, 256, 256, 1, 1, cases.CUS)
    finally:
        lib.sage_set_deterministic(was)
    for alt in cases.ALTERNATIVES["backward"]:
        assert any(alt in s for s in seen), alt
    assert lib.sage_backward_kernel_name_at(4160, 4160, 256, 256, 1, 1, 256, 1 << 9, ctypes.create_string_buffer(256), 256) == _lib.ERR_INVALID
    assert lib.sage_backward_kernel_name_at(4160, 4160, 256, 256, 1, 1, 256, cases.B_INDEXED, ctypes.create_string_buffer(256), 256) == _lib.ERR_INVALID
    assert lib.sage_forward_kernel_name_at(4160, 256, 256, 256, 1 << 6, ctypes.create_string_buffer(96), 96) == _lib.ERR_INVALID


def test_pairwise_table(lib):
    from graphpope_amd import _lib
    seen = []
    for row, table in cases.PAIRWISE.items():
        lib.pope_debug_set(_lib.KNOB_PAIRWISE_KERNEL, row[6])
        try:
            old = _name(lib.pope_pairwise_kernel_name, *row[:6], cases.CUS)
            assert pairwise_at(lib, row, 0) == old == pw.CASES[row], row
            for mask, want in table.items():
                got = pairwise_at(lib, row, mask)
                assert got == want, (row, mask)
                # a misaligned A means nothing to a call that reads the anchors through their ids
                assert (got != old) == (not (mask == cases.P_A and row[5])), (row, mask)
                seen.append(got)
        finally:
            lib.pope_debug_set(_lib.KNOB_PAIRWISE_KERNEL, 0)
    assert set(cases.PAIRWISE_GPU_ROWS) <= {r for r in pw.CASES if r[0] <= pw.GPU_MAX_N}
    for alt in cases.ALTERNATIVES["pairwise"]:
        assert any(alt in s for s in seen), alt
    assert any(s.endswith("k_minmax_apply") for s in seen)
    assert lib.pope_pairwise_kernel_name_at(257, 128, 256, 8, 1, 0, 256, 1 << 5, ctypes.create_string_buffer(256), 256) == _lib.ERR_INVALID


def test_finalize_table(lib):
    from graphpope_amd import _lib
    n, k, f = cases.FINALIZE_SHAPE
    seen = []
    for (has_x, mask), want in cases.FINALIZE.items():
        assert finalize_at(lib, has_x, mask) == want, (has_x, mask)
        assert finalize_at(lib, has_x, 0) == _name(lib.pope_finalize_kernel_name, n, k, f, has_x, 1) == cases.FINALIZE[(has_x, 0)]
        seen.append(want)
    for alt in cases.ALTERNATIVES["finalize"]:
        assert alt in seen
    assert lib.pope_finalize_kernel_name_at(n, k, f, 1, 1, 4, ctypes.create_string_buffer(64), 64) == _lib.ERR_INVALID


def test_the_adam_bound_is_a_bound_on_a_float32_numpy_step():
    """The restatement and its bound against update() written out in NumPy float32 (no fused multiply-add): every element within the bound,
    a NaN gradient element poisons its own three results and nothing else."""
    rs = np.random.RandomState(3)
    n = 5000
    f32 = np.float32
    p, g = rs.randn(n).astype(f32), (rs.randn(n) * 0.1).astype(f32)
    m, v = (rs.randn(n) * 0.01).astype(f32), (rs.rand(n) * 1e-3).astype(f32)
    g[17] = np.nan
    v[5], g[5] = 0.0, 0.0
    for wd in (0.0, 0.01):
        lr, b1, b2, eps, step = 1e-3, 0.9, 0.999, 1e-8, 3
        want, bound = cases.adam_reference(p, g, m, v, lr, b1, b2, eps, wd, step)
        s, c = f32(lr / (1.0 - b1 ** step)), f32(1.0 / np.sqrt(1.0 - b2 ** step))
        G = g + f32(wd) * p if wd else g
        m1 = m + (G - m) * f32(1.0 - b1)
        v1 = f32(b2) * v + f32(1.0 - b2) * G * G
        p1 = p - s * (m1 / (np.sqrt(v1) * c + f32(eps)))
        for k, got in (("p", p1), ("m", m1), ("v", v1)):
            assert got.dtype == f32
            nan = np.isnan(got)
            assert nan.sum() == 1 and nan[17] and np.array_equal(nan, np.isnan(want[k]))
            ratio = cases.worst_ratio(got, want[k], bound[k])
            assert 0 < ratio <= 1.0, (k, wd, ratio)
