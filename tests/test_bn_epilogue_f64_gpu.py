"""The fused BatchNorm1d + ReLU + dropout epilogue on the GPU (csrc/epilogue.hip) against the NumPy float64 reference, the restated
dropout mask and the float32-rounding bounds of tests/bn_epilogue_cases.py -- main.py:207-209.

Every case is one forward and one backward call through the library's own entry points (raw pointers: the only way to reach the
scalar path of a misaligned operand, a device extent with a sentinel behind it, or hand-made external partials).  Each test prints
its worst error-to-bound ratios (DESIGN.md records them)."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import bn_epilogue_cases as bn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


def _place(arr, dev, shifted=False):
    """`arr` on the device; shifted: as a view that starts one element (4 bytes) into its buffer."""
    t = torch.as_tensor(arr)
    if not shifted:
        out = t.to(dev)
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=dev)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _forward_args(case, dev):
    cap, c = case.x.shape
    t = {"x": _place(case.x, dev, case.misalign == "x"), "dy": _place(case.dy, dev), "gamma": _place(case.gamma, dev, case.misalign == "gamma"),
         "beta": _place(case.beta, dev),
         "rm": None if case.no_running else _place(case.running_mean, dev), "rv": None if case.no_running else _place(case.running_var, dev),
         "nbt": torch.zeros(1, dtype=torch.int64, device=dev),
         "y": torch.full((cap, c), float(bn.SENTINEL), device=dev), "gx": torch.full((cap, c), float(bn.SENTINEL), device=dev),
         "mean": _place(np.zeros(c, np.float32), dev, case.misalign == "save_mean"), "rstd": torch.zeros(c, device=dev),
         "gg": torch.zeros(c, device=dev), "gb": torch.zeros(c, device=dev),
         "rows_dev": None if case.rows is None else torch.tensor([case.rows], dtype=torch.int32, device=dev),
         "seed_dev": None}
    if case.seed_dev is not None:                                      # a uint64 word, as int64 bits
        v = case.seed_dev - (1 << 64) if case.seed_dev >= 1 << 63 else case.seed_dev
        t["seed_dev"] = torch.tensor([v], dtype=torch.int64, device=dev)
    return t


def run_case(lib, dev, case):
    """Forward + backward of `case`; the dict tests/bn_epilogue_cases.check takes."""
    from graphpope_amd._lib import check, ptr
    cap, c = case.x.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = _forward_args(case, dev)
    scratch = torch.empty(lib.sage_bn_scratch_bytes(c), dtype=torch.uint8, device=dev)
    head = (ptr(t["x"]), cap, c, ptr(t["gamma"]), ptr(t["beta"]), ptr(t["rm"]), ptr(t["rv"]), ptr(t["nbt"]), bn.MOMENTUM, bn.EPS,
            int(case.training), case.p, case.seed, ptr(t["y"]), ptr(t["mean"]), ptr(t["rstd"]), ptr(scratch), scratch.numel(),
            ptr(t["rows_dev"]), ptr(t["seed_dev"]))
    if case.ext_rows_per_part:
        pa, pb = (torch.as_tensor(a, device=dev) for a in bn.external_partials(case))
        check(lib.sage_bn_relu_dropout_forward_stats(*head, ptr(pa), ptr(pb), pa.shape[0], case.ext_rows_per_part, stream))
    else:
        check(lib.sage_bn_relu_dropout_forward(*head, stream))
    check(lib.sage_bn_relu_dropout_backward(ptr(t["x"]), ptr(t["dy"]), cap, c, ptr(t["gamma"]), ptr(t["beta"]), ptr(t["mean"]), ptr(t["rstd"]),
                                            int(case.training), case.p, case.seed, ptr(t["gx"]), ptr(t["gg"]), ptr(t["gb"]), ptr(scratch),
                                            scratch.numel(), ptr(t["rows_dev"]), ptr(t["seed_dev"]), stream))
    assert int(t["nbt"]) == (1 if case.training else 0), case.name      # num_batches_tracked + 1 in training mode only
    host = {k: None if v is None else v.cpu().numpy() for k, v in t.items()}
    return {"save_mean": host["mean"], "save_rstd": host["rstd"], "running_mean": host["rm"], "running_var": host["rv"], "y": host["y"],
            "grad_x": host["gx"], "grad_beta": host["gb"], "grad_gamma": host["gg"]}


def _run_family(dev, cases, title):
    from graphpope_amd import _lib
    lib = _lib.load()
    worst, failures = {}, []
    for case in cases:
        try:
            bn.merge(worst, bn.check(case, bn.reference(case), run_case(lib, dev, case)))
        except AssertionError as e:                                    # every case is reported, not only the first
            failures.append(str(e)[:300])
    print(f"{title}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])


def test_slab_and_column_block_edges_in_every_mode(dev):
    """Twenty (M, C) pairs -- the slab count reaching 256, 16 -> 17 rows per slab, a second trip of the four-rows-in-flight loop; the
    scalar and the 16-byte path with a second column block each -- in training mode with p = 0 and 0.5 and in eval mode; p = 1 and
    running statistics left out once."""
    _run_family(dev, bn.shape_cases(), "shapes")


def test_off_centre_columns_keep_the_float64_sums_bounds(dev):
    """Columns of spread 1 at offsets up to +-1000 and a constant column: E[x^2] - E[x]^2 over float64 sums stays inside the
    conditioning bound; float32 accumulators would miss it by orders of magnitude."""
    _run_family(dev, bn.off_centre_cases(), "off-centre")


def test_a_misaligned_operand_takes_the_scalar_path_with_the_same_results(dev):
    """x, gamma or save_mean one element into its buffer at a C that is a multiple of 4: same bounds and the same restated mask as
    the aligned call."""
    _run_family(dev, bn.misaligned_cases(), "misaligned")


def test_device_extents_leave_the_rows_behind_them_alone(dev):
    """rows_dev below the capacity: the statistics and sums are those of the true rows (the rest of x and dy is NaN), y and grad_x
    keep their sentinel behind them, the mask index does not depend on the extent; once with seed_dev."""
    _run_family(dev, bn.extent_cases(), "extents")


def test_external_first_stage_partials(dev):
    """sage_bn_relu_dropout_forward_stats on float64 partials made in NumPy, 625 parts included; with a device extent the parts behind
    the true row count hold NaN and are not read; the three-launch call on the same input meets the same bounds; partials that do not
    cover the rows are refused."""
    from graphpope_amd import _lib
    cases = bn.external_cases()
    _run_family(dev, cases, "external")
    _run_family(dev, [dataclasses.replace(c, ext_rows_per_part=None) for c in cases], "external (three launches)")
    lib = _lib.load()
    case = cases[2]                                                    # 17 rows in tiles of 16: one part does not cover them
    t = _forward_args(case, dev)
    scratch = torch.empty(lib.sage_bn_scratch_bytes(5), dtype=torch.uint8, device=dev)
    pa, pb = (torch.as_tensor(a, device=dev) for a in bn.external_partials(case))
    code = lib.sage_bn_relu_dropout_forward_stats(_lib.ptr(t["x"]), 17, 5, _lib.ptr(t["gamma"]), _lib.ptr(t["beta"]), _lib.ptr(t["rm"]), _lib.ptr(t["rv"]),
                                                  _lib.ptr(t["nbt"]), bn.MOMENTUM, bn.EPS, 1, case.p, case.seed, _lib.ptr(t["y"]), _lib.ptr(t["mean"]),
                                                  _lib.ptr(t["rstd"]), _lib.ptr(scratch), scratch.numel(), None, None, _lib.ptr(pa), _lib.ptr(pb), 1, 16,
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == _lib.ERR_INVALID and int(t["nbt"]) == 0 and bool((t["y"] == float(bn.SENTINEL)).all())
