"""The float64 reference, the bounds and the cases of tests/loss_head_cases.py, checked without a GPU: the reference equals torch's
float64 F.cross_entropy (main.py:216) to 1e-12, torch's float32 one sits within half of the loss bound and a quarter of the gradient
bound (so the bounds are reachable by a float32 implementation), the non-finite expectations are torch's, the case lists hold what
their names claim, and graphpope_amd.sage.cross_entropy refuses logits that are not float32."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_head_cases as lh


def _all_cases():
    return [case for build in lh.FAMILIES.values() for case in build()] + lh.eval_agreement_cases()


def _torch(case, dtype):
    """(row losses, gradient of their sum, mean loss) of F.cross_entropy in `dtype` on the CPU; bad labels become ignored ones."""
    c = case.logits.shape[1]
    y = case.y.copy()
    y[(y < 0) | (y >= c)] = case.ignore_index
    x = torch.tensor(case.logits, dtype=dtype, requires_grad=True)
    yt = torch.tensor(y)
    rows = F.cross_entropy(x, yt, ignore_index=case.ignore_index, reduction="none")
    rows.sum().backward()
    with torch.no_grad():
        mean = F.cross_entropy(x, yt, ignore_index=case.ignore_index)
    return rows.detach().numpy(), x.grad.numpy(), float(mean)


def test_reference_equals_torch_float64():
    for case in _all_cases():
        if not np.isfinite(case.logits).all():
            continue
        ref = lh.reference(case.logits, case.y, case.ignore_index)
        rows, grad, mean = _torch(case, torch.float64)
        k = ref.counted
        scale = max(1.0, float(np.abs(case.logits).max()))            # lse - x_y cancels numbers of the logits' size (1e6 in the shifted case)
        assert np.abs(rows[k] - ref.loss[k]).max(initial=0.0) <= 1e-12 * scale, case.name
        assert np.abs(grad - ref.grad).max() <= 1e-12 * scale, case.name
        assert (np.isnan(mean) and ref.count == 0) or abs(mean - ref.mean) <= 1e-12 * scale, case.name
        assert not rows[~k].any() and not grad[~k].any()


def test_torch_float32_sits_inside_the_bounds_with_headroom():
    """Half of the loss bound, 2^-21 on the unscaled gradient: scales 1e-3 to 3e4 and C from 1 to 1000, and every finite case."""
    cases = [c for c in _all_cases() if np.isfinite(c.logits).all()]
    for c in (1, 2, 7, 65, 513, 1000):
        for scale in (1e-3, 1.0, 80.0, 3e3, 3e4):
            rng = np.random.RandomState(c)
            cases.append(lh.Case(f"C={c} scale {scale}", (rng.randn(64, c) * scale).astype(np.float32), rng.randint(0, c, 64).astype(np.int64)))
    worst_row = worst_grad = 0.0
    for case in cases:
        ref = lh.reference(case.logits, case.y, case.ignore_index)
        rows, grad, mean = _torch(case, torch.float32)
        k = ref.counted
        if k.any():
            r = float((np.abs(rows[k].astype(np.float64) - ref.loss[k]) / ref.loss_bound[k]).max())
            g = float(np.abs(grad[k].astype(np.float64) - ref.grad[k]).max() / lh.GRAD_ABS)
            worst_row, worst_grad = max(worst_row, r), max(worst_grad, g)
            assert r <= 0.5, (case.name, r)
            assert g <= 0.25, (case.name, g)
            assert abs(mean - ref.mean) <= ref.mean_bound, case.name
    print(f"torch float32 on the CPU: worst row loss {worst_row:.3f} of its bound, worst gradient {worst_grad:.3f} of 2^-19")


def test_non_finite_expectations_are_torchs():
    seen = set()
    for case in lh.non_finite_cases():
        ref = lh.reference(case.logits, case.y, case.ignore_index)
        rows, grad, mean = _torch(case, torch.float32)
        kind = case.name.split(" ", 2)[2]
        seen.add(kind)
        assert ref.count == 8 and float(ref.inv_count) == 0.125
        if np.isfinite(ref.mean):
            assert abs(mean - ref.mean) <= ref.mean_bound, (case.name, mean, ref.mean)
        else:
            assert lh._same_kind(mean, ref.mean), (case.name, mean, ref.mean)
        k = ref.counted                                                # (torch's log_softmax backward leaves 0 * NaN in an ignored row)
        assert np.array_equal(np.isnan(grad[k]), np.isnan(ref.grad[k])), case.name
        want = {"nan counted": np.nan, "nan ignored": None, "+inf counted": np.nan, "-inf off label": None, "-inf at label": np.inf,
                "row of -inf": np.nan}[kind]
        if want is None:
            assert np.isfinite(ref.mean) and np.isfinite(ref.grad).all()
        else:
            assert lh._same_kind(ref.mean, want)
        if kind == "-inf off label":
            assert ref.grad[4, 3] == 0.0 and ref.grad[4, 64] == 0.0 and grad[4, 3] == 0.0
        if kind == "-inf at label":
            assert np.isfinite(ref.grad).all() and ref.grad[4, 7] == -1.0
        if kind in ("nan counted", "+inf counted", "row of -inf"):
            assert np.isnan(ref.grad[4]).all() and np.isfinite(np.delete(ref.grad, 4, axis=0)).all()
    assert seen == set(lh.NON_FINITE_KINDS)


def test_case_lists_hold_what_they_claim():
    cols = lh.column_cases()
    assert [c.logits.shape[1] for c in cols[:-1]] == list(lh.COLUMNS) and cols[-1].logits.shape == (257, 513) and 6 in cols[-1].forms
    ref = lh.reference(cols[0].logits, cols[0].y)                     # C = 1: loss 0, gradient 0
    assert not ref.loss[ref.counted].any() and not ref.grad.any()
    rows = lh.row_cases()
    assert sorted({c.logits.shape[0] for c in rows}) == sorted(lh.ROWS + (16390,))
    shapes_456 = {c.logits.shape for fam in lh.FAMILIES.values() for c in fam() if 4 in c.forms and "non-finite" not in c.name}
    assert shapes_456 == set(lh.OPTIMISER_SHAPES)
    for case in rows:
        n = case.logits.shape[0]
        edges = lh.edge_rows(n)
        assert 0 in edges and n - 1 in edges and all(k - 1 in edges and (k == n or k in edges) for k in range(256, n + 1, 256))
        ignored = case.y[edges] == -100
        assert np.array_equal(ignored[1:], ~ignored[:-1])             # alternately ignored and counted
    assert {bool(c.y[0] == -100) for c in rows if c.logits.shape[0] == 2049} == {True, False}
    for case in lh.magnitude_cases():
        ref = lh.reference(case.logits, case.y)
        live = np.flatnonzero(ref.counted)
        assert ref.count > 200 and np.isfinite(ref.loss[live]).all()
        x = case.logits.astype(np.float64)
        other = x.copy()
        other[live, case.y[live]] = -np.inf
        lead = x[live, case.y[live]] - other[live].max(axis=1)
        if case.name.endswith("confident"):
            assert lead.min() >= 30.0 and np.array_equal(case.exact_zero_rows, live) and ref.loss[live].max() < 1e-10
        elif case.name.endswith("trails by 200"):
            assert np.abs(lead + 200.0).max() < 1e-3 and np.abs(ref.loss[live] + lead).max() < 10.0 and (ref.grad[live, case.y[live]] == -1.0).all()
        elif case.name.endswith("all equal"):
            assert np.abs(ref.loss[live] - np.log(x.shape[1])).max() < 1e-12
    for case in lh.label_cases():
        ref = lh.reference(case.logits, case.y, case.ignore_index)
        if "ignore_index" in case.name:
            assert ref.bad == 0 and 0 < ref.count < case.y.size and 0 <= case.ignore_index < case.logits.shape[1]
        elif "all ignored" in case.name:
            assert ref.count == 0 and np.isnan(ref.mean) and ref.inv_count == 0 and not ref.grad.any() and ref.bad == 0
        else:
            assert ref.bad == 1 and not ref.grad[[0, 17, 36]].any() and not ref.counted[[0, 17, 36]].any()


def test_check_rejects_what_the_kernel_used_to_return():
    """The checker itself: a result that drops the NaN row (finite mean over seven rows, 1 / 7) fails; the reference's own passes."""
    case = lh.non_finite_cases()[0]
    ref = lh.reference(case.logits, case.y)
    rows = np.where(ref.counted, ref.loss, -1.0).astype(np.float32)
    good = {"loss": ref.mean, "inv_count": ref.inv_count, "bad": 0, "rows": rows, "grad": ref.grad.astype(np.float32), "grad_scale": 1.0}
    lh.check(case, ref, good, "reference")
    dropped = dict(good, loss=float(np.nanmean(ref.loss[ref.counted])))
    with pytest.raises(AssertionError):
        lh.check(case, ref, dropped, "NaN row dropped")
    with pytest.raises(AssertionError):
        lh.check(case, ref, dict(good, inv_count=np.float32(1) / np.float32(7)), "count without the NaN row")


def test_cross_entropy_refuses_logits_that_are_not_float32():
    from graphpope_amd.sage import cross_entropy
    y = torch.zeros(4, dtype=torch.int64)
    for dtype in (torch.float64, torch.bfloat16, torch.float16):
        with pytest.raises(ValueError):
            cross_entropy(torch.zeros(4, 3, dtype=dtype), y)
    with pytest.raises(RuntimeError):                                  # float32 on the CPU gets past the checks to the device check
        cross_entropy(torch.zeros(4, 3), y)
