"""The conditions that keep test_pairwise_conditioning_gpu.py honest, checked without a GPU: every case of
pairwise_cases.py is in the regime its name claims, and the reference alone passes the bounds the kernel is held to.

Measured on the CPU (the figures the bounds come from): euclidean, max |scale(oracle.pairwise) - scale64(ref64)| over all
cases 3.5e-7 (D = 100, mu = 30; bound 1e-6); cosine metrics, the oracle's own float32 deviation reaches 8.7e-4 at mu = 30,
D = 260 (bound 2e-3, only there to catch a broken generator: the GPU test uses the deviation itself).
"""
import numpy as np
import pytest

import pairwise_cases as pc

NAMES = [c.name for c in pc.CASES]


def test_the_case_list_is_the_one_the_kernels_need():
    by = {(c.n, c.k, c.d, c.mu) for c in pc.CASES}
    for mu in (0, 2, 4, 6, 8, 9, 9.9, 12, 30):
        assert (700, 65, 128, mu) in by
    for d in (36, 100, 132, 129, 260):
        for mu in (0, 6, 9.9, 30):
            assert (700, 65, d, mu) in by
    assert (700, 257, 128, 9.9) in by and (33, 5, 4, 9.9) in by
    # the derived offsets: at the kernel's threshold, and 1.54 x / 2.7 x above it
    assert abs(1.0 / (pc.MU_STRADDLE ** 2 + 1) / pc.CANCEL_RATIO - 1.0) < 0.05
    assert all(1.3 < 1.0 / (mu ** 2 + 1) / pc.CANCEL_RATIO < 3.0 for mu in pc.MU_JUST_ABOVE)
    for regime in ("far", "just_above", "straddle", "all_below"):
        assert any(c.regime == regime for c in pc.CASES), regime


@pytest.mark.parametrize("name", NAMES)
def test_anchors_are_table_rows_with_one_repeat(name):
    i = pc.inputs(name)
    assert i.emb.dtype == np.float32 and i.emb.shape == (i.case.n, i.case.d)
    assert i.anchors.shape == (i.case.k,) and len(np.unique(i.anchors)) == i.case.k - 1
    assert i.anchors.min() >= 0 and i.anchors.max() < i.case.n


@pytest.mark.parametrize("name", NAMES)
def test_regime_of_each_case(name):
    i = pc.inputs(name)
    ratio = pc.ratio64(i.emb, i.anchors)
    pairs = ratio[~pc.coincident(i.emb, i.anchors)]
    below = float((pairs < pc.CANCEL_RATIO).mean())
    just = float(((pairs > pc.CANCEL_RATIO) & (pairs <= pc.JUST_ABOVE_MAX)).mean())
    print(f"{name}: ratio min {pairs.min():.4g} median {np.median(pairs):.4g} max {pairs.max():.4g}; "
          f"below {100 * below:.2f} %, just above {100 * just:.2f} %")
    regime = i.case.regime
    if regime == "far":
        assert pairs.min() > pc.FAR_RATIO
    elif regime == "just_above":
        assert just >= 0.95
    elif regime == "straddle":
        assert 0.20 <= below <= 0.80
    elif regime == "all_below":
        assert below >= 0.99
    else:
        assert regime is None


@pytest.mark.parametrize("name", NAMES)
def test_euclidean_reference_is_far_inside_the_gate(name, oracle):
    i = pc.inputs(name)
    got = oracle.minmax_scale_columns(oracle.pairwise(i.emb, i.emb[i.anchors], "euclidean"))
    err = float(np.abs(got - pc.want64(name, "euclidean")).max())
    print(f"{name}: oracle against float64, euclidean: {err:.3g}")
    assert err <= 1e-6


@pytest.mark.parametrize("fn", ["distance", "similarity"])
@pytest.mark.parametrize("name", NAMES)
def test_cosine_reference_deviation(name, fn, oracle):
    i = pc.inputs(name)
    got = oracle.minmax_scale_columns(oracle.pairwise(i.emb, i.emb[i.anchors], fn))
    dev = float(np.abs(got - pc.want64(name, fn)).max())
    print(f"{name}: oracle against float64, {fn}: {dev:.3g}")
    assert np.isfinite(dev) and dev < 2e-3


@pytest.mark.parametrize("name", NAMES)
def test_exact_column_properties_hold_for_the_reference(name, oracle):
    """What the GPU test asserts without a tolerance: every scaled column has the minimum 0.0; for `euclidean` and
    `distance` (raw minimum ~0, shift ~0) the maximum is within one ulp of 1.  `similarity` is excluded from the second:
    its raw minimum is ~0.99 on an off-centre table and fl(max * scale) is rounded at the size of max * scale."""
    i = pc.inputs(name)
    for fn in pc.FNS:
        s = oracle.minmax_scale_columns(oracle.pairwise(i.emb, i.emb[i.anchors], fn))
        assert (s.min(axis=0) == 0.0).all()
        if fn != "similarity":
            assert (np.abs(s.max(axis=0).astype(np.float64) - 1.0) <= 2.0 ** -23).all()


@pytest.mark.parametrize("d", [128, 129])
def test_degenerate_rows_are_zero_rows_for_the_reference(d, oracle):
    emb, anchors = pc.degenerate_table(d)
    assert not emb[3].any() and (emb[11] == np.float32(1e-25)).all() and float(np.float32(1e-25) ** 2) == 0.0
    assert anchors.shape == (pc.K,) and anchors[0] == 3 and anchors[1] == 11 and anchors[-1] == 3
    sim = oracle.pairwise(emb, emb[anchors], "similarity")
    dist = oracle.pairwise(emb, emb[anchors], "distance")
    assert np.isfinite(sim).all() and np.isfinite(dist).all()
    assert np.abs(sim[[3, 11]]).max() < 1e-20 and np.abs(sim[:, [0, 1, -1]]).max() < 1e-20
    assert (dist[[3, 11]] == 1.0).all() and (dist[:, [0, 1, -1]] == 1.0).all()
    for fn in pc.FNS:
        assert np.isfinite(oracle.minmax_scale_columns(oracle.pairwise(emb, emb[anchors], fn))).all()
