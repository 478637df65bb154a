"""Every path of the node2vec-space call's plan (csrc/pairwise.hip: pairwise_plan) on the GPU: each row of pairwise_plan_cases.CASES with
n <= GPU_MAX_N runs under its knob, in both anchor forms (row ids; the gathered rows), all three metrics.  The row's own form first asserts
the path -- pope_pairwise_kernel_name must print the row's string -- then the values: out[:, :f] is x bit for bit, and the embedding
columns are within the project's gate, 1e-5 absolute on the scaled values, of float64 (pairwise_cases.ref64 / scale64) on a zero-mean table
with one coincident row pair whose twin is an anchor (the euclidean fix-up runs in every case).

The shapes are the smallest at which each path can go wrong: n = 257 (289 where k = 260 anchors have to be rows of the table) leaves a
ragged last tile for the 32-row and the 64-row tile kernel, k = 257 / 260 a second column group of the persistent kernel and a third of
the one-tile kernel with one / four live columns, d = 128, 36, 132, 7 the full, the zero-padded, the too deep and the unvectorised row,
f = 0, 8, 6, 4100 no copy, the fused copies, the odd width and the row wider than the side copy takes.
"""
import ctypes

import numpy as np
import pytest
import torch

import pairwise_cases as pc
import pairwise_plan_cases as cases

pytestmark = pytest.mark.gpu
ATOL = 1e-5
ROWS = [row for row in cases.CASES if row[0] <= cases.GPU_MAX_N]


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "n%d_d%d_k%d_f%d_x%d_id%d_knob%d" % r)
def test_every_plan_row_against_float64(row, dev):
    from graphpope_amd import _lib, engine
    n, d, k, f, has_x, by_id, knob = row
    lib = _lib.load()
    emb, anchors = cases.inputs(n, d, k)
    emb_d = torch.as_tensor(np.array(emb), device=dev)             # copies: the shared inputs are read-only arrays
    rows_d = torch.as_tensor(emb[anchors], device=dev)
    x = pc.features(n, f) if has_x else None
    x_d = torch.as_tensor(x, device=dev) if has_x else None
    buf = ctypes.create_string_buffer(256)
    lib.pope_debug_set(_lib.KNOB_PAIRWISE_KERNEL, knob)
    try:
        _lib.check(lib.pope_pairwise_kernel_name(n, d, k, f, has_x, by_id, cases.CUS, buf, 256))
        assert buf.value.decode() == cases.CASES[row]
        for fn in pc.FNS:
            want = cases.want64(n, d, k, fn)
            first = None
            for form in ("ids", "rows"):
                ids, rows = (anchors, None) if form == "ids" else (None, rows_d)
                if has_x:
                    out = engine.pairwise_features(x_d, emb_d, ids, fn, anchor_embeddings=rows).cpu().numpy()
                else:                                               # the embedding columns at c0 = f of a matrix of f + k columns
                    wide = torch.zeros((n, f + k), dtype=torch.float32, device=dev)
                    out = engine.pairwise_embedding(emb_d, ids, fn, anchor_embeddings=rows, out=wide, c0=f).cpu().numpy()
                tag = f"{row} {fn} {form}"
                assert out.dtype == np.float32 and out.shape == (n, f + k), tag
                if has_x:
                    assert np.array_equal(bits(out[:, :f]), bits(x)), tag
                else:
                    assert not out[:, :f].any(), tag
                got = out[:, f:]
                assert np.isfinite(got).all(), tag
                err = float(np.abs(got - want).max())
                print(f"{tag}: max error {err:.3g}")
                assert err <= ATOL, tag
                if fn == "euclidean":                               # the anchor's own row and its twin: recomputed, exactly 0
                    assert got[5, 0] == 0.0 and got[7, 0] == 0.0, tag
                if first is None:
                    first = got
                assert np.array_equal(bits(got), bits(first)), tag  # both anchor forms read the same rows and do the same arithmetic
    finally:
        lib.pope_debug_set(_lib.KNOB_PAIRWISE_KERNEL, 0)
