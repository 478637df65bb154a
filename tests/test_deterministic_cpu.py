"""Deterministic mode without a GPU: the switch, what sage_backward_kernel_name and sage_conv_scratch_bytes say under it, and the
argument checks of sage_scatter_mean_det (include/graphpope_hip.h).  Host logic only; every test leaves the switch off."""
import ctypes

import numpy as np
import pytest

import sage_backward_cases as cases
from graphpope_amd import _lib

SUM = "k_scatter_sum_det"
INDEX = "k_det_clear+k_det_index<false>+k_det_scan+k_det_index<true>+" + SUM
GONE = ("k_scatter_mean", "k_scatter_and_finals", "k_zero_rows")


@pytest.fixture
def lib():
    lib = _lib.load()
    assert lib.sage_get_deterministic() == 0, "an earlier test left the switch on"
    yield lib
    lib.sage_set_deterministic(0)
    null = ctypes.c_void_p(0)
    lib.sage_scatter_mean_det(null, null, 0, 0, 0, null, 1, null, null, 0, null, null)     # an empty call: leaves no message behind


def _name(lib, shape, extra, grad_x, grad_b):
    n_dst, c_in, c_out = shape
    buf = ctypes.create_string_buffer(256)
    _lib.check(lib.sage_backward_kernel_name(n_dst, n_dst + extra, c_in, c_out, int(grad_x), int(grad_b), cases.CUS, buf, 256))
    return buf.value.decode()


def test_the_switch_returns_the_previous_value_and_round_trips(lib):
    assert lib.sage_set_deterministic(1) == 0 and lib.sage_get_deterministic() == 1
    assert lib.sage_set_deterministic(1) == 1
    assert lib.sage_set_deterministic(7) == 1 and lib.sage_get_deterministic() == 1       # any non-zero value is "on"
    assert lib.sage_set_deterministic(0) == 1 and lib.sage_get_deterministic() == 0
    assert lib.sage_set_deterministic(0) == 0


def test_python_switch_and_context_manager_restore_the_previous_value(lib):
    from graphpope_amd import sage
    assert sage.is_deterministic() is False
    assert sage.set_deterministic(True) is False and sage.is_deterministic() is True
    with sage.deterministic(False):
        assert sage.is_deterministic() is False
        with sage.deterministic():
            assert sage.is_deterministic() is True
        assert sage.is_deterministic() is False
    assert sage.is_deterministic() is True
    with pytest.raises(ZeroDivisionError):
        with sage.deterministic(False):
            1 / 0
    assert sage.is_deterministic() is True                                           # restored on the way out of an exception too
    assert sage.set_deterministic(False) is True and lib.sage_get_deterministic() == 0


@pytest.mark.parametrize("extra", [0, 300])
def test_names_with_the_switch_off_are_the_pinned_ones(lib, extra):
    for shape in cases.PATHS:
        assert _name(lib, shape, extra, True, True) == cases.expected_name(shape, extra), shape
        if None not in cases.PATHS[shape]:                          # (the table holds the tiles a refused dual path would take)
            for grad_x, grad_b in ((True, False), (False, True), (False, False)):
                assert _name(lib, shape, extra, grad_x, grad_b) == cases.expected_name(shape, extra, grad_x, grad_b), (shape, grad_x, grad_b)


@pytest.mark.parametrize("extra", [0, 300])
def test_names_with_the_switch_on(lib, extra):
    """With an input gradient: neither zeroing nor scatter, and the index build + sum behind the twin GEMM of every path; the weight and
    bias gradients' kernels are the ones of the default mode.  Without an input gradient: the same names in both modes."""
    for shape in cases.PATHS:
        for grad_b in (True, False):
            off_x, off_nox = _name(lib, shape, extra, True, grad_b), _name(lib, shape, extra, False, grad_b)
            lib.sage_set_deterministic(1)
            try:
                on_x, on_nox = _name(lib, shape, extra, True, grad_b), _name(lib, shape, extra, False, grad_b)
            finally:
                lib.sage_set_deterministic(0)
            assert on_nox == off_nox, (shape, grad_b)
            assert not any(k in on_x for k in GONE), (shape, on_x)
            vec = "true" if shape[1] % 4 == 0 else "false"
            assert on_x.endswith("+" + INDEX + "<%s>" % vec), (shape, on_x)
            # what stands in front is the default chain without its zeroing and scatter (dual: with the plain reductions)
            front = on_x[:-len("+" + INDEX + "<%s>" % vec)]
            want = off_x.replace("k_scatter_and_finals", "k_bwd_finals").replace("+k_zero_rows", "").replace("+k_scatter_mean", "")
            assert front == want, (shape, on_x, off_x)


def test_scratch_with_the_switch_on_holds_the_index_as_well(lib):
    for shape in cases.PATHS:
        n_dst, c_in, c_out = shape
        for extra, nnz in ((0, 0), (300, 5000), (300, 1)):
            off = lib.sage_conv_scratch_bytes(n_dst + extra, n_dst, nnz, c_in, c_out)
            index = lib.sage_scatter_mean_det_scratch_bytes(n_dst + extra, n_dst, nnz)
            assert index >= 4 * (n_dst + extra + 1) + 2 * 4 * nnz
            lib.sage_set_deterministic(1)
            try:
                on = lib.sage_conv_scratch_bytes(n_dst + extra, n_dst, nnz, c_in, c_out)
            finally:
                lib.sage_set_deterministic(0)
            assert on == off + index and on >= off
            assert lib.sage_conv_scratch_bytes(n_dst + extra, n_dst, nnz, c_in, c_out) == off
    assert lib.sage_scatter_mean_det_scratch_bytes(0, 0, 0) == 0
    assert lib.sage_scatter_mean_det_scratch_bytes(10, 11, 5) == 0                    # refused sizes ask for nothing
    assert lib.sage_scatter_mean_det_scratch_bytes(10, 5, -1) == 0


def test_scatter_mean_det_checks_its_arguments_before_any_hip_call(lib):
    """Null pointers, n_dst > n_src, c <= 0, negative sizes and too little scratch: POPE_ERR_INVALID with the function's name in the
    message -- on a machine without a device, so no HIP call can have come first.  The empty call and a block with neither an edge nor
    a row behind its destinations have nothing to launch and return OK."""
    host = (ctypes.c_int32 * 64)()
    p = ctypes.cast(host, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    n_src, n_dst, nnz, c = 12, 8, 20, 4
    room = lib.sage_scatter_mean_det_scratch_bytes(n_src, n_dst, nnz)
    good = [p, p, n_src, n_dst, nnz, p, c, p, p, room, null, null]

    def refused(**change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        assert lib.sage_scatter_mean_det(*args) == _lib.ERR_INVALID, change
        assert b"sage_scatter_mean_det" in lib.pope_last_error(), change

    for at in (0, 1, 5, 7, 8):                                                       # rowptr, col, grad_agg, grad_x, scratch
        refused(**{"a%d" % at: null})
    refused(a3=n_src + 1)                                                             # n_dst > n_src
    refused(a6=0)
    refused(a6=-4)
    refused(a2=-1, a3=-1)
    refused(a4=-1)
    refused(a2=2 ** 31 - 1)
    refused(a9=room - 1)
    refused(a9=0)
    # the empty call takes null pointers, as every entry point of the library does
    assert lib.sage_scatter_mean_det(null, null, 0, 0, 0, null, c, null, null, 0, null, null) == _lib.OK and lib.pope_last_error() == b""
    assert lib.sage_scatter_mean_det(null, null, 0, 0, 0, null, 0, null, null, 0, null, null) == _lib.ERR_INVALID    # ... but not c = 0
    # no edge, and no row behind the destinations: nothing to add, nothing to overwrite
    room0 = lib.sage_scatter_mean_det_scratch_bytes(n_dst, n_dst, 0)
    assert lib.sage_scatter_mean_det(p, null, n_dst, n_dst, 0, p, c, p, p, room0, null, null) == _lib.OK and lib.pope_last_error() == b""


def test_backward_refuses_a_scratch_sized_with_the_switch_off(lib):
    """sage_conv_backward checks its scratch against sage_conv_scratch_bytes under the CURRENT mode: a buffer sized before the switch
    went on is refused (POPE_ERR_WORKSPACE) instead of being overrun by the index."""
    host = (ctypes.c_float * 16)()
    p = ctypes.cast(host, ctypes.c_void_p)
    n_src, n_dst, nnz, c_in, c_out = 40, 30, 100, 8, 4
    off = lib.sage_conv_scratch_bytes(n_src, n_dst, nnz, c_in, c_out)
    lib.sage_set_deterministic(1)
    try:
        rc = lib.sage_conv_backward(p, p, n_src, n_dst, nnz, p, p, c_in, p, p, c_out, p, p, p, p, p, p, off, None, None)
        assert rc == _lib.ERR_WORKSPACE and b"sage_conv_backward" in lib.pope_last_error()
    finally:
        lib.sage_set_deterministic(0)


def test_reference_restatement_of_the_contract_on_a_tiny_block():
    """The NumPy loop the GPU tests compare with (tests/deterministic_cases.py), checked here against a hand computation."""
    import deterministic_cases as det
    rowptr = np.array([0, 2, 2, 5], dtype=np.int32)                                  # degrees 2, 0, 3
    col = np.array([3, 0, 3, 3, 1], dtype=np.int32)                                  # destination 2 lists source 3 twice
    gagg = np.array([[1.0], [99.0], [3.0]], dtype=np.float32)
    gx = np.array([[10.0], [20.0], [30.0], [-7.0], [-7.0]], dtype=np.float32)        # rows 3, 4: behind the destinations
    out = det.scatter_mean_reference(rowptr, col, 5, 3, gagg, gx)
    third = np.float32(3.0) * (np.float32(1.0) / np.float32(3.0))
    half = np.float32(0.5)
    assert out[0, 0] == np.float32(10.0) + half and out[1, 0] == np.float32(20.0) + third and out[2, 0] == np.float32(30.0)
    assert out[3, 0] == (np.float32(0.0) + half + third) + third and out[4, 0] == 0.0 and not np.signbit(out[4, 0])
    assert gx[3, 0] == -7.0                                                          # the input is not modified
