"""CPU-side checks of the boundary: the C-ABI library loads and exports every symbol of include/graphpope_hip.h."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "graphpope_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b((?:pope|sage)_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from graphpope_amd import _lib
    lib = _lib.load()
    declared = _declared_symbols()
    assert len(declared) >= 15
    for query in ("sage_forward_kernel_name", "sage_backward_kernel_name", "pope_pairwise_kernel_name", "pope_finalize_kernel_name"):
        assert query in declared and query + "_at" in declared      # every plan query and its sibling that takes the alignment mask
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(_lib.SIGNATURES) == declared            # the ctypes table and the header agree


def test_size_queries_need_no_gpu():
    from graphpope_amd import _lib
    lib = _lib.load()
    assert lib.pope_version().startswith(b"graphpope_hip")
    assert [lib.pope_words(k) for k in (1, 64, 65, 128, 129, 130, 256, 257, 1024)] == [1, 1, 2, 2, 4, 4, 4, 8, 16]
    assert lib.pope_plane_bytes(89250, 256) == 89250 * 4 * 8
    assert lib.pope_bfs_scratch_bytes(89250, 899756, 256) >= 2 * 89250 * 4 * 8
    assert lib.pope_csr_scratch_bytes(89250, 899756) >= (89250 + 1) * 4
    assert lib.pope_last_error() == b""


def test_product_path_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from graphpope_amd import engine
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.require_gpu()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "graphpope_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("SURVEY", ""), f


def test_argument_validation_needs_no_gpu():
    """Bad sizes / null pointers are rejected before any HIP call, with a message behind pope_last_error()."""
    from graphpope_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    assert lib.pope_csr_build(null, 5, -1, null, null, null, null, null, 0, 0, null) == _lib.ERR_INVALID
    assert b"pope_csr_build" in lib.pope_last_error()
    assert lib.pope_geodesic_finalize(null, 0, 10, 4, null, 0, null, 4, 0, null) == _lib.ERR_INVALID
    assert lib.pope_pairwise_minmax(null, 10, 4, null, 2, 7, null, 2, 0, null, 0, null) == _lib.ERR_INVALID
    assert lib.sage_conv_forward(null, null, 5, 9, 0, null, 4, null, null, null, 4, null, null, null, 0, null, null) == _lib.ERR_INVALID
    assert lib.pope_geodesic_run_workspace_bytes(10, 10, 0, 8) == 0 and lib.pope_geodesic_run_workspace_bytes(89250, 899756, 256, 8) > 0
    assert lib.sage_bn_relu_dropout_forward(null, 8, 4, null, null, null, null, null, 0.1, 1e-5, 1, 0.5, 0, null, null, null, null, 0, null, null, null) == _lib.ERR_INVALID
    assert lib.sage_bn_relu_dropout_backward(null, null, 8, 4, null, null, null, null, 1, 0.5, 0, null, null, null, null, 0, null, null, null) == _lib.ERR_INVALID
    assert lib.sage_adam_step(2, null, null, null, null, null, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, null, null) == _lib.ERR_INVALID
    assert lib.sage_adam_step(0, null, null, null, null, null, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, null, null) == _lib.ERR_INVALID      # step is 1-based
    assert lib.pope_geodesic_column_stats(null, 3, 10, 4, null, null, null, 0, null) == _lib.ERR_INVALID
    assert lib.sage_sample_batch_device(null, null, 10, null, 4, null, 2, 0, null, null, null, null, null, null, 0, null) == _lib.ERR_INVALID
    assert lib.sage_advance_counters(null, null, 3, null) == _lib.ERR_INVALID and lib.sage_copy_segments(2, null, null, null, null) == _lib.ERR_INVALID
    assert lib.pope_assemble_host_result(null, 0, 0, null, 0, 0, null, 0, 4, 1, 0, null) == _lib.ERR_INVALID
    assert lib.pope_host_pin(null, 0) == _lib.ERR_INVALID
    assert lib.sage_bn_scratch_bytes(256) > 0 and lib.pope_column_stats_scratch_bytes(256) > 0
    import pytest
    with pytest.raises(_lib.PopeError, match="null pointer"):
        _lib.check(lib.pope_concat(null, 4, 4, null, 8, null))


def test_result_tensor_pool_reuses_the_pages_of_a_freed_result(monkeypatch):
    """engine.host_result_tensor: pageable, contiguous, handed back when the LAST view dies, reused only for the same size,
    dropped for another size and when GRAPHPOPE_RESULT_POOL_MB forbids keeping it."""
    import torch
    from graphpope_amd import engine
    engine._RESULT_POOL.clear()
    t = engine.host_result_tensor(1000, 700)
    assert t.shape == (1000, 700) and t.dtype == torch.float32 and t.is_contiguous() and not t.is_pinned() and not t.is_shared()
    p = t.data_ptr()
    t.fill_(3.0)
    v = t[:, :4]
    del t
    assert not engine._RESULT_POOL                       # a view still uses the pages
    del v
    assert list(engine._RESULT_POOL) == [2800000]
    t2 = engine.host_result_tensor(1000, 700)
    assert t2.data_ptr() == p and not engine._RESULT_POOL
    t3 = engine.host_result_tensor(1000, 700)            # the pool is empty: fresh pages
    assert t3.data_ptr() != p
    del t2, t3
    assert list(engine._RESULT_POOL) == [2800000]        # one entry, the first to come back
    t4 = engine.host_result_tensor(2000, 700)            # another size evicts it
    assert not engine._RESULT_POOL
    monkeypatch.setenv("GRAPHPOPE_RESULT_POOL_MB", "1")
    del t4
    assert not engine._RESULT_POOL                       # 5.6 MB > 1 MB: unmapped, not kept
    monkeypatch.setenv("GRAPHPOPE_RESULT_POOL_MB", "0")
    t5 = engine.host_result_tensor(1000, 700)            # pool off: torch's own allocation
    del t5
    assert not engine._RESULT_POOL
    assert engine.host_result_tensor(3, 5).shape == (3, 5)


def test_kernel_name_queries_follow_the_shapes():
    """pope_level_kernel_name / pope_finalize_kernel_name are host logic (which instantiation a shape gets: bench.py and the profiles label
    their roofline entries with them): the shapes of BASELINE configs[1], [3], [4] and of their per-rank shards, no GPU needed."""
    import ctypes
    from graphpope_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)

    def level(n, k):
        _lib.check(lib.pope_level_kernel_name(n, k, buf, 64))
        return buf.value.decode()

    def fin(n, k, f, shards):
        _lib.check(lib.pope_finalize_kernel_name(n, k, f, 1 if f else 0, shards, buf, 64))
        return buf.value.decode()

    flickr, rmat = 89250, 1 << 22
    assert level(flickr, 256) == "k_bfs_level<4, 1, 0>" and level(flickr, 128) == "k_bfs_level<2, 1, 0>"
    assert level(flickr, 1024) == "k_bfs_level<8, 1, 2>" and level(flickr, 768) == "k_bfs_level<4, 1, 2>"
    assert level(rmat, 512) == "k_bfs_level<8, 3, 0>" and level(rmat, 64) == "k_bfs_level<1, 3, 0>"
    assert level(rmat, 1024) == "k_bfs_level<8, 3, 1>" and level(rmat, 768) == "k_bfs_level<4, 3, 1>"
    assert fin(flickr, 256, 500, 1) == "k_finalize_pipe<2, 1>" and fin(flickr, 1024, 500, 1) == "k_finalize_wide<2>"
    assert fin(rmat, 512, 0, 1) == "k_finalize_lut" and fin(flickr, 256, 500, 8) == "k_finalize_wide<2>" and fin(rmat, 64, 0, 8) == "k_finalize_lut"
    assert lib.pope_level_kernel_name(0, 256, buf, 64) != 0 and lib.pope_finalize_kernel_name(flickr, 0, 0, 0, 1, buf, 64) != 0


# K -> (WT, TILES) of k_bfs_level<WT, LIVE, TILES> with the live table in LDS (LIVE = 1) and read from global memory (LIVE = 2 or 3):
# csrc/geodesic.hip, level_plan.  17 distinct kernels: every instantiation the library holds.
LEVEL_TABLE = {40: ((1, 0), (1, 0)), 100: ((2, 0), (2, 0)), 200: ((4, 0), (4, 0)), 300: ((8, 2), (8, 0)), 600: ((4, 2), (4, 1)), 1000: ((8, 2), (8, 1))}


def level_kernel_wanted(k, mode):
    wt, tiles = LEVEL_TABLE[k][0 if mode == 1 else 1]
    return "k_bfs_level<%d, %d, %d>" % (wt, mode, tiles)


def test_level_kernel_table_under_every_live_mode():
    """pope_level_kernel_name is level_plan printed: every (anchor count, POPE_KNOB_LIVE_MODE) cell of the table at a node count small
    enough for the LDS table -- all 17 level kernels -- and the two limits at which a requested mode gives way: mode 1 above 256 Ki nodes
    (the table no longer fits LDS: 3), mode 3 where the summary exceeds 48 KB (above 12 582 912 nodes: 2).  No GPU needed."""
    import ctypes
    from graphpope_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)

    def level(n, k):
        _lib.check(lib.pope_level_kernel_name(n, k, buf, 64))
        return buf.value.decode()

    seen = set()
    try:
        for mode in (1, 2, 3):
            assert lib.pope_debug_set(_lib.KNOB_LIVE_MODE, mode) == _lib.OK
            for k in LEVEL_TABLE:
                assert level(4096, k) == level_kernel_wanted(k, mode), (k, mode)
                seen.add(level(4096, k))
        assert len(seen) == 17
        lib.pope_debug_set(_lib.KNOB_LIVE_MODE, 1)
        assert level(256 * 1024, 200) == "k_bfs_level<4, 1, 0>" and level(256 * 1024 + 1, 200) == "k_bfs_level<4, 3, 0>"
        assert level(256 * 1024 + 1, 1000) == "k_bfs_level<8, 3, 1>"
        lib.pope_debug_set(_lib.KNOB_LIVE_MODE, 3)
        assert level(12582912, 300) == "k_bfs_level<8, 3, 0>" and level(12582912 + 1, 300) == "k_bfs_level<8, 2, 0>"
        lib.pope_debug_set(_lib.KNOB_LIVE_MODE, -1)
        assert level(12582912 + 1, 600) == "k_bfs_level<4, 2, 1>" and level(4096, 600) == "k_bfs_level<4, 1, 2>"
        lib.pope_debug_set(_lib.KNOB_LIVE_MODE, 4)                       # no such mode, no such kernel: an error, not another kernel
        assert lib.pope_level_kernel_name(4096, 200, buf, 64) == _lib.ERR_INVALID and b"k_bfs_level<4, 4, 0>" in lib.pope_last_error()
    finally:
        lib.pope_debug_set(_lib.KNOB_LIVE_MODE, -1)


def test_finalize_kernel_names_under_the_variant_knob():
    """pope_finalize_kernel_name is finalize_plan printed, under POPE_KNOB_FINALIZE_VARIANT too: 0 the generic kernel (one shard), 7 the
    round 1-3 kernel; 9 asks for the table kernel with features as well, which needs the separate feature copy -- where that copy cannot
    take the shape (an output of 4 GiB or more: 32-bit byte offsets) the launch falls back to k_finalize_wide, and so does the name."""
    import ctypes
    from graphpope_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)

    def fin(n, k, f, shards):
        _lib.check(lib.pope_finalize_kernel_name(n, k, f, 1 if f else 0, shards, buf, 64))
        return buf.value.decode()

    flickr, rmat = 89250, 1 << 22
    try:
        lib.pope_debug_set(_lib.KNOB_FINALIZE_VARIANT, 0)
        assert fin(flickr, 256, 500, 1) == "k_finalize<true>" and fin(flickr, 256, 501, 1) == "k_finalize<false>"
        assert fin(rmat, 64, 0, 8) == "k_finalize_fast"                  # several shards in one launch: never the generic kernel
        lib.pope_debug_set(_lib.KNOB_FINALIZE_VARIANT, 7)
        assert fin(flickr, 256, 500, 1) == "k_finalize_fast" and fin(rmat, 64, 0, 8) == "k_finalize_fast"
        assert fin(flickr, 256, 501, 1) == "k_finalize<false>"
        lib.pope_debug_set(_lib.KNOB_FINALIZE_VARIANT, 9)
        assert fin(flickr, 1024, 500, 1) == "k_finalize_lut"             # 89 250 x 1 524 floats: the copy kernel takes it
        assert fin(rmat, 512, 256, 1) == "k_finalize_wide<1>"            # 4 194 304 x 768 floats = 12 GiB: it cannot
        assert fin(rmat, 512, 0, 1) == "k_finalize_lut"
    finally:
        lib.pope_debug_set(_lib.KNOB_FINALIZE_VARIANT, 1)
        lib.pope_debug_set(_lib.KNOB_FINALIZE_VARIANT, 8)
        lib.pope_debug_set(_lib.KNOB_FINALIZE_VARIANT, 11)


def test_sage_forward_kernel_name_follows_the_shapes_and_the_knobs():
    """sage_forward_kernel_name is the forward projection's own plan function (csrc/sage.hip: forward_plan) printed: which kernels a layer
    of a shape launches on 256 CUs, by default, with the gather not beside the projection, and without the whole-tile kernels.  Host
    logic, no GPU needed.  The retired knob numbers are unknown knobs."""
    import ctypes
    from graphpope_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(96)

    def name(n_dst, c_in, c_out):
        _lib.check(lib.sage_forward_kernel_name(n_dst, c_in, c_out, 256, buf, 96))
        return buf.value.decode()

    def beside(r, b=4):
        return "k_gather_beside_gemm<%d>+k_gemm_tile16<%d, %d>" % (r, r, b)

    def tile16(r, b=4):
        return "k_gemm_tile16<%d, %d>" % (r, b)

    streamk = "k_gemm_streamk_ld<32>"
    # shape: (default, POPE_KNOB_SAGE_FORWARD_OVERLAP = 0, POPE_KNOB_FORWARD_WHOLE_TILES = 0)
    table = {
        (5800, 256, 256): (beside(3), tile16(3), streamk),
        (8100, 200, 256): (beside(4), tile16(4), streamk),
        (9988, 756, 256): (beside(5), tile16(5), streamk),
        (9988, 756, 250): (beside(5), tile16(5), streamk),
        (12200, 132, 256): (tile16(6), tile16(6), streamk),
        (11000, 256, 256): (tile16(6), tile16(6), streamk),
        (13000, 256, 256): (tile16(7), tile16(7), streamk),
        (14300, 128, 200): (streamk, streamk, streamk),
        (4096, 256, 256): (streamk, streamk, streamk),
        (2000, 64, 128): (tile16(1), tile16(1), "k_gemm<64, 64>"),
        (700, 40, 24): ("k_gemm<64, 64>",) * 3,
        (300, 64, 64): ("k_gemm<64, 64>",) * 3,
        (9988, 757, 256): ("k_gemm<64, 64>",) * 3,               # depth not a multiple of 4
        (15000, 757, 256): ("k_gemm<64, 128>",) * 3,
        (70000, 30, 600): ("k_gemm<128, 256>",) * 3,
    }
    settings = [(None, None), (_lib.KNOB_SAGE_FORWARD_OVERLAP, 0), (_lib.KNOB_FORWARD_WHOLE_TILES, 0)]
    try:
        for column, (knob, value) in enumerate(settings):
            if knob is not None:
                assert lib.pope_debug_set(knob, value) == _lib.OK
            for shape, want in table.items():
                assert name(*shape) == want[column], (shape, column)
            if knob is not None:
                assert lib.pope_debug_set(knob, 1) == _lib.OK
        assert lib.pope_debug_set(_lib.KNOB_GEMM_TILE16_BUFFERS, 3) == _lib.OK
        assert name(5800, 256, 256) == beside(3, 3) and name(11000, 256, 256) == tile16(6, 3) and name(2000, 64, 128) == tile16(1, 3)
    finally:
        lib.pope_debug_set(_lib.KNOB_SAGE_FORWARD_OVERLAP, 1)
        lib.pope_debug_set(_lib.KNOB_FORWARD_WHOLE_TILES, 1)
        lib.pope_debug_set(_lib.KNOB_GEMM_TILE16_BUFFERS, 4)
    assert lib.pope_debug_set(3, 7) == _lib.ERR_INVALID and lib.pope_debug_set(15, 0) == _lib.ERR_INVALID
    assert lib.sage_forward_kernel_name(0, 256, 256, 256, buf, 96) == _lib.ERR_INVALID


def test_sage_backward_kernel_name_pins_the_path_of_every_tested_shape():
    """sage_backward_kernel_name is the backward pass's own plan function (csrc/sage.hip: backward_plan) printed, in launch order: pinned on
    256 CUs at the benchmark's layer shapes and at every case of tests/test_sage_backward_gpu.py -- each of those shapes is the smallest
    that reaches its path, so a retune that moves one shows here.  Host logic, no GPU needed."""
    import ctypes
    import sage_backward_cases as cases
    from graphpope_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)

    def name(n_dst, n_src, c_in, c_out, grad_x=True, grad_b=True, cap=256):
        _lib.check(lib.sage_backward_kernel_name(n_dst, n_src, c_in, c_out, int(grad_x), int(grad_b), cases.CUS, buf, cap))
        return buf.value.decode()

    for (n_dst, n_src, c_in, c_out, grad_x), want in cases.BASELINE_NAMES.items():
        assert name(n_dst, n_src, c_in, c_out, grad_x) == want, (n_dst, c_in, c_out)
    table = cases.HOST_CASES + cases.EXTENT_CASES + cases.ROUNDING_CASES
    assert len({c["id"] for c in table}) == len(table)
    seen = set()
    try:
        for c in table:
            lib.pope_debug_set(_lib.KNOB_STREAMK_XCD, 1 if c["xcd"] else 0)
            n_dst, c_in, c_out = c["shape"]
            got = name(n_dst, n_dst + c["extra"], c_in, c_out, c["grad_x"], c["grad_b"])
            assert got == cases.expected_name(c["shape"], c["extra"], c["grad_x"], c["grad_b"], c["xcd"]), c["id"]
            seen.update(got.split("+"))
    finally:
        lib.pope_debug_set(_lib.KNOB_STREAMK_XCD, 1)
    # every launch of conv_backward_impl (k_gather_rows, in front of the indexed twin cases, has no name of its own) ...
    for kernel in ("k_gemm_streamk_tn<32>[xcd]", "k_gemm_streamk_tn<32>", "k_streamk_tn_fixup<32>", "k_colsum_partial<true>", "k_colsum_partial<false>",
                   "k_colsum_final", "k_gemm_dual<64, 64, 2, 2>[splits=16]", "k_scatter_and_finals", "k_bwd_finals", "k_slab_reduce", "k_zero_rows",
                   "k_scatter_mean", "k_gemm<64, 64, 2, 2, 2, 2>[splits=5]", "k_gemm<64, 64, 2, 2, 2, 2>", "k_gemm<64, 64, 2, 2, 0, 0>[splits=3]",
                   "k_gemm<64, 128, 2, 2, 0, 0>[splits=25]", "k_gemm<64, 64, 2, 2, 1, 2>", "k_gemm<64, 128, 2, 2, 1, 2>", "k_gemm<128, 256, 4, 1, 1, 2>"):
        assert kernel in seen or kernel == "k_bwd_finals", kernel
    # ... k_bwd_finals only without edges, which the query does not take: the dual cases with nnz = 0 reach it
    assert any(not c["edges"] and cases.PATHS[c["shape"]][0] == "dual" for c in table)
    assert name(4065, 4065, 256, 256) != name(4064, 4064, 256, 256)
    assert lib.sage_backward_kernel_name(0, 5, 4, 4, 1, 1, 256, buf, 256) == _lib.ERR_INVALID
    assert lib.sage_backward_kernel_name(9, 5, 4, 4, 1, 1, 256, buf, 256) == _lib.ERR_INVALID          # destinations are the first sources
    assert lib.sage_backward_kernel_name(4065, 4065, 256, 256, 1, 1, 256, buf, 16) == _lib.ERR_INVALID and b"do not fit" in lib.pope_last_error()
    assert name(1, 1, 4, 4) == cases.expected_name((1, 4, 4), 0)                                       # (clears the error string)


def test_sage_scratch_size_queries_keep_their_recorded_values():
    """sage_conv_scratch_bytes, sage_conv_backward_indexed_scratch_bytes, sage_scatter_mean_det_scratch_bytes and
    sage_conv_forward_indexed_scratch_bytes at every layer of the backward tests and of the benchmark, deterministic mode off and on, equal
    tests/golden/sage_scratch_sizes.json: values recorded (tools/sage_scratch_sizes.py) from the library as it was before the scratch layout
    moved into one function, so callers that size their buffers once keep working.  Host logic, no GPU needed."""
    import json
    import sys
    import sage_backward_cases as cases
    from graphpope_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import sage_scratch_sizes as tool
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "sage_scratch_sizes.json")))
    assert golden["queries"] == list(tool.QUERIES)
    assert [tuple(r["args"]) for r in golden["rows"]] == cases.size_query_args()       # the table covers today's shapes, each once
    assert len(golden["rows"]) >= 30
    lib = _lib.load()
    was = lib.sage_set_deterministic(0)
    try:
        for row in golden["rows"]:
            for mode, key in ((0, "off"), (1, "on")):
                lib.sage_set_deterministic(mode)
                assert tool.sizes(lib, row["args"]) == row[key], (row["args"], key)
    finally:
        lib.sage_set_deterministic(was)


def test_pairwise_kernel_name_pins_the_plan_of_every_case():
    """pope_pairwise_kernel_name is the node2vec-space call's own plan function (csrc/pairwise.hip: pairwise_plan) printed, in launch order:
    pinned at every row of tests/pairwise_plan_cases.py, whose strings were written down from the launch code before the plan existed.
    Host logic, no GPU needed."""
    import ctypes
    import pairwise_plan_cases as cases
    from graphpope_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)

    def name(n, d, k, f, has_x, by_id, cap=256):
        _lib.check(lib.pope_pairwise_kernel_name(n, d, k, f, has_x, by_id, cases.CUS, buf, cap))
        return buf.value.decode()

    seen = set()
    try:
        for (n, d, k, f, has_x, by_id, knob), want in cases.CASES.items():
            assert lib.pope_debug_set(_lib.KNOB_PAIRWISE_KERNEL, knob) == _lib.OK
            got = name(n, d, k, f, has_x, by_id)
            assert got == want, (n, d, k, f, has_x, by_id, knob)
            seen.update(got.split("+"))
    finally:
        lib.pope_debug_set(_lib.KNOB_PAIRWISE_KERNEL, 0)
    # every step of the plan that has a name
    assert seen == {"pope_concat", "k_gather_anchor_rows", "k_sqnorm<true>", "k_sqnorm<false>", "k_pairwise<1>", "k_pairwise<1>[copy]", "k_pairwise<0>",
                    "k_pairwise<0>[copy]", "k_pairwise_persistent[sets=1]", "k_pairwise_persistent[sets=2]", "k_copy_features", "k_minmax_fold",
                    "k_minmax_reduce", "k_minmax_finish", "k_minmax_apply", "k_minmax_apply4"}
    assert sum(n <= cases.GPU_MAX_N for (n, *_rest) in cases.CASES) >= 30
    assert name(257, 128, 256, 8, 1, 0, cap=100) == cases.CASES[257, 128, 256, 8, 1, 0, 0]             # 71 characters and the terminator fit 100
    for bad in ((0, 128, 256, 8, 1, 0), (257, 0, 256, 8, 1, 0), (257, 128, 0, 8, 1, 0), (257, 128, 256, -1, 1, 0), (2 ** 31, 128, 256, 8, 1, 0)):
        assert lib.pope_pairwise_kernel_name(*bad, cases.CUS, buf, 256) == _lib.ERR_INVALID, bad
    assert lib.pope_pairwise_kernel_name(257, 128, 256, 8, 1, 0, 0, buf, 256) == _lib.ERR_INVALID
    assert lib.pope_pairwise_kernel_name(257, 128, 256, 8, 1, 0, cases.CUS, None, 256) == _lib.ERR_INVALID
    assert lib.pope_pairwise_kernel_name(257, 128, 256, 8, 1, 0, cases.CUS, buf, 16) == _lib.ERR_INVALID and b"do not fit" in lib.pope_last_error()
    assert name(33, 4, 5, 0, 0, 1) == cases.CASES[33, 4, 5, 0, 0, 1, 0]                                # (clears the error string)


def test_pairwise_scratch_size_queries_keep_their_recorded_values():
    """pope_pairwise_scratch_bytes and pope_pairwise_by_id_scratch_bytes at SCRATCH_SHAPES of tests/pairwise_plan_cases.py equal
    tests/golden/pairwise_scratch_sizes.json: values recorded (tools/pairwise_scratch_sizes.py) from the library as it was before the
    scratch layout moved into one function, so callers that size their buffers once keep working.  Host logic, no GPU needed."""
    import json
    import sys
    import pairwise_plan_cases as cases
    from graphpope_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import pairwise_scratch_sizes as tool
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pairwise_scratch_sizes.json")))
    assert golden["queries"] == list(tool.QUERIES)
    assert [tuple(r["args"]) for r in golden["rows"]] == cases.SCRATCH_SHAPES
    lib = _lib.load()
    for row in golden["rows"]:
        assert tool.sizes(lib, row["args"]) == row["bytes"], row["args"]
    by_shape = {tuple(r["args"]): r["bytes"] for r in golden["rows"]}
    assert by_shape[257, 256, 0] == [by_shape[257, 256, 128][0], 0] and by_shape[0, 256, 128] == [0, 0] and by_shape[257, 0, 128] == [0, 0]
    assert by_shape[89250, 256, 128][1] == by_shape[89250, 256, 128][0] + 256 * 128 * 4             # the gathered anchor rows


def test_exact_family_of_the_sage_backward_tests_is_exact():
    """The inputs of every exact case of tests/test_sage_backward_gpu.py, at every true size it runs: all partial sums of the weight and
    bias gradients are integers below 2^24 and those of grad_x multiples of 2^-7 below 2^17, so float32 adds them without rounding in any
    order and the device results can be compared bit for bit."""
    import sage_backward_cases as cases
    done, visits = set(), 0
    for c in cases.HOST_CASES + cases.EXTENT_CASES:
        for n in c["trues"] or (c["shape"][0],):
            visits += 1
            key = cases.reference_key(c, n)
            if key in done:                                            # (the inputs are a function of the key alone)
                continue
            ref = cases.reference(c, n)
            ref.assert_exact_family_is_exact()
            assert ref.nnz > 0 or not c["edges"]
            if c["edges"]:
                assert (ref.deg == 128).any()
            done.add(key)
    # every run of every case went through the loop, and every distinct set of inputs was checked: the 18 shapes with and without
    # extra sources and with no edges, and each extent case's true sizes
    distinct = {cases.reference_key(c, n) for c in cases.HOST_CASES + cases.EXTENT_CASES for n in c["trues"] or (c["shape"][0],)}
    assert done == distinct and len(done) >= 2 * len(cases.PATHS) + 8 + 2 * 13 and visits >= len(cases.HOST_CASES) + 2 * len(cases.EXTENT_CASES)
    for c in cases.EXTENT_CASES:
        assert all(cases.reference_key(c, n) in done for n in c["trues"]) and len(c["trues"]) >= 2
    # the forward extent runs of the same file
    forward = {(n, c_in, c_out) for (cap, c_in, c_out), _, _ in cases.FORWARD for n in cases.forward_trues(cap)}
    assert len(forward) == 7                                          # (700 of 4160 and 700 of 5800 share their inputs)
    for key in sorted(forward):
        cases.forward_reference(*key).assert_exact_family_is_exact()
