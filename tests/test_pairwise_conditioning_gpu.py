"""Accuracy of the node2vec-space path on OFF-CENTRE tables against float64 (cases and references: pairwise_cases.py; the
conditions that make these checks meaningful: test_pairwise_cases_cpu.py).

On zero-mean data d2 ~ |x|^2 + |a|^2 and the float32 expansion d2 = |x|^2 + |a|^2 - 2 x.a loses nothing; rows that share
an offset put the euclidean epilogue just above, across and below its cancellation threshold.  Every case runs through
every kernel path it can reach (POPE_KNOB_PAIRWISE_KERNEL 0-3 for D <= 128 in 16-byte rows, else the one-tile-per-block
kernel) and through both anchor forms (row ids; the gathered rows), with F = 8 and F = 3 feature columns.

Bounds.  euclidean: the project's gate, 1e-5 absolute on the scaled values, against scale64(ref64) -- the reference holds
it with 30 x to spare.  Cosine metrics: scikit-learn computes them in float32 and itself drifts from float64 on these
tables (1e-5 at mu = 4, 9e-4 at mu = 30), so the kernel is held to max(1e-5, 2 x the oracle's deviation on the same case);
kernel and reference are float32 dot products summed in different orders; measured quotients 0.77-1.35 on the N = 700
tables, 1.75 on the 33 x 5 one.  Measured euclidean errors: up to 5.7e-5 with the threshold 1e-2
(15 cases failed), 3.6e-6 with 2^-3 (profiles/pairwise_conditioning_before.txt, _after.txt).
"""
import numpy as np
import pytest
import torch

import pairwise_cases as pc

pytestmark = pytest.mark.gpu
ATOL = 1e-5
NAMES = [c.name for c in pc.CASES]
NAN_BITS = 0x7FC0BEEF                                  # a quiet NaN with a payload: the guard pattern
ONE_ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


def kernel_paths(d):
    return (0, 1, 2, 3) if d <= 128 and d % 4 == 0 else (0,)


class forced_kernel:
    def __init__(self, kernel):
        from graphpope_amd import _lib
        self.lib, self.knob, self.kernel = _lib.load(), _lib.KNOB_PAIRWISE_KERNEL, kernel

    def __enter__(self):
        self.lib.pope_debug_set(self.knob, self.kernel)

    def __exit__(self, *exc):
        self.lib.pope_debug_set(self.knob, 0)


def run_forms(emb, anchors, fn, dev):
    """{(form, F): [N, F + K] float32} for the anchor-id form and the gathered-rows form, F = 8 and F = 3 (F = 3: the
    separate feature copy and the scalar scaling pass)."""
    from graphpope_amd import engine
    emb_d = torch.as_tensor(np.array(emb), device=dev)        # a copy: the shared inputs are read-only arrays
    rows_d = torch.as_tensor(emb[anchors], device=dev)
    out = {}
    for f in (8, 3):
        x_d = torch.as_tensor(pc.features(emb.shape[0], f), device=dev)
        out["ids", f] = engine.pairwise_features(x_d, emb_d, anchors, fn).cpu().numpy()
        out["rows", f] = engine.pairwise_features(x_d, emb_d, None, fn, anchor_embeddings=rows_d).cpu().numpy()
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("fn", pc.FNS)
@pytest.mark.parametrize("name", NAMES)
def test_off_centre_tables_against_float64(name, fn, dev, oracle):
    i = pc.inputs(name)
    emb, anchors, k = i.emb, i.anchors, i.case.k
    want = pc.want64(name, fn)
    if fn == "euclidean":
        tol = ATOL
    else:
        ref_dev = float(np.abs(oracle.minmax_scale_columns(oracle.pairwise(emb, emb[anchors], fn)) - want).max())
        tol = max(ATOL, 2.0 * ref_dev)
    for kernel in kernel_paths(i.case.d):
        with forced_kernel(kernel):
            outs = run_forms(emb, anchors, fn, dev)
        first = None
        for (form, f), out in outs.items():
            tag = f"{name} {fn} kernel {kernel} {form} F={f}"
            assert out.dtype == np.float32 and out.shape == (i.case.n, f + k), tag
            assert np.array_equal(bits(out[:, :f]), bits(pc.features(i.case.n, f))), tag     # the feature columns, bit for bit
            got = out[:, f:]
            assert np.isfinite(got).all(), tag
            err = float(np.abs(got - want).max())
            print(f"{tag}: max error {err:.3g} (bound {tol:.3g})")
            assert err <= tol, tag
            # min * s + (0 - min * s) is exactly 0; with a column minimum of 0 the shift is 0 and max * fl(1 / max) is one
            # rounding from 1 (`similarity` has no zero minimum: fl(max * s) is rounded at the size of max * s, and the
            # reference's own maximum is up to 512 ulp from 1 on these tables, test_pairwise_cases_cpu.py)
            assert (got.min(axis=0) == 0.0).all(), tag
            if fn != "similarity":
                assert (np.abs(got.max(axis=0).astype(np.float64) - 1.0) <= ONE_ULP).all(), tag
            if fn == "euclidean":                       # the own row: recomputed as a sum of squared differences, 0 * s + (0 - 0 * s)
                assert (got[anchors, np.arange(k)] == 0.0).all(), tag
            # both anchor forms read the same rows and do the same arithmetic
            if first is None:
                first = got
            assert np.array_equal(bits(got), bits(first)), tag


@pytest.mark.parametrize("k", [65, 64])
@pytest.mark.parametrize("fn", pc.FNS)
def test_guard_columns_around_the_embedding(fn, k, dev):
    """pairwise_embedding into columns [5, 5 + K) of a wider matrix pre-filled with a NaN pattern: the columns in front and
    behind keep their bits, the K columns in between are the plain call's (K = 64: the plain call scales four columns per
    lane, the call at c0 = 5 one; both are also run at c0 = 4 in a matrix whose width is a multiple of 4)."""
    from graphpope_amd import engine
    i = pc.inputs(f"n700_k65_d128_mu{pc.MU_STRADDLE:g}_straddle")
    emb_d = torch.as_tensor(np.array(i.emb), device=dev)
    anchors = np.array(i.anchors[:k])
    plain = engine.pairwise_embedding(emb_d, anchors, fn).cpu().numpy()
    wide = torch.full((i.case.n, 5 + k + 3), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    got = engine.pairwise_embedding(emb_d, anchors, fn, out=wide, c0=5)
    assert got.data_ptr() == wide.data_ptr()
    w = wide.cpu().numpy()
    assert (bits(w[:, :5]) == NAN_BITS).all() and (bits(w[:, 5 + k:]) == NAN_BITS).all()
    assert np.array_equal(bits(w[:, 5:5 + k]), bits(plain))
    wide4 = torch.full((i.case.n, 4 + k + 4 + (-k) % 4), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    engine.pairwise_embedding(emb_d, anchors, fn, out=wide4, c0=4)
    w4 = wide4.cpu().numpy()
    assert (bits(w4[:, :4]) == NAN_BITS).all() and (bits(w4[:, 4 + k:]) == NAN_BITS).all()
    assert np.array_equal(bits(w4[:, 4:4 + k]), bits(plain))
    if fn == "euclidean":
        assert np.abs(plain - pc.scale64(pc.ref64(i.emb, anchors, fn))).max() <= ATOL


@pytest.mark.parametrize("d", [128, 129])
@pytest.mark.parametrize("fn", pc.FNS)
def test_zero_and_underflowing_rows(fn, d, dev, oracle):
    """An exact zero row and a row whose squares underflow float32 (components 1e-25), both also anchors: the reference
    treats both as zero rows (similarity 0, distance 1); a factor 1 / sqrt((float)|r|^2) = inf would give 0 * inf = NaN."""
    emb, anchors = pc.degenerate_table(d)
    want = oracle.minmax_scale_columns(oracle.pairwise(emb, emb[anchors], fn))
    for kernel in kernel_paths(d):
        with forced_kernel(kernel):
            outs = run_forms(emb, anchors, fn, dev)
        for (form, f), out in outs.items():
            tag = f"d={d} {fn} kernel {kernel} {form} F={f}"
            got = out[:, f:]
            assert np.isfinite(got).all(), tag
            err = float(np.abs(got - want).max())
            print(f"{tag}: max error {err:.3g}")
            assert err <= ATOL, tag
