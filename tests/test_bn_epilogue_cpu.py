"""tests/bn_epilogue_cases.py checked without a GPU: the float64 reference equals torch's float64 BatchNorm1d + relu + the restated
mask through autograd (main.py:207-209) to 1e-12; a NumPy float32 restatement of the documented formulas sits within HALF of
every bound the kernels are held to (so the bounds are reachable, and were not sized from a kernel's output); elements on the ReLU
gate are at most 1e-3 of every case; the mask restatement has the keep rate it claims and depends on both words of the seed."""
import numpy as np
import torch

import bn_epilogue_cases as bn


def _all_cases():
    return [case for build in bn.FAMILIES.values() for case in build()]


def test_reference_equals_torch_float64_autograd():
    for case in _all_cases():
        m, c = case.m, case.x.shape[1]
        ref = bn.reference(case)
        mod = torch.nn.BatchNorm1d(c, eps=float(np.float32(bn.EPS)), momentum=float(np.float32(bn.MOMENTUM))).double()
        with torch.no_grad():
            mod.weight.copy_(torch.tensor(case.gamma, dtype=torch.float64))
            mod.bias.copy_(torch.tensor(case.beta, dtype=torch.float64))
            mod.running_mean.copy_(torch.tensor(case.running_mean, dtype=torch.float64))
            mod.running_var.copy_(torch.tensor(case.running_var, dtype=torch.float64))
        mod.train(case.training)
        x = torch.tensor(case.x[:m], dtype=torch.float64, requires_grad=True)
        if m == 1 and case.training:                                   # torch refuses one row per channel; the formulas are plain there
            assert np.abs(ref.var).max() == 0.0 and np.abs(ref.dx).max() == 0.0
            continue
        keep = torch.tensor(bn.keep_mask(case.seed, m, c, case.p if case.training else 0.0, case.seed_dev or 0))
        y = torch.relu(mod(x)) * keep * bn.inv_keep(case.training, case.p)
        y.backward(torch.tensor(case.dy[:m], dtype=torch.float64))
        scale = max(1.0, float(np.abs(case.x[:m]).max()))                 # x - mu cancels numbers of the inputs' size (1e3 off centre)
        for name, got, want in (("y", y.detach(), ref.y), ("dx", x.grad, ref.dx), ("dgamma", mod.weight.grad, ref.dgamma),
                                ("dbeta", mod.bias.grad, ref.dbeta)):
            err = float(np.abs(got.numpy() - want).max())
            assert err <= 1e-12 * scale * max(1.0, float(np.abs(want).max())), (case.name, name, err)
        if case.training and not case.no_running:
            assert np.abs(mod.running_mean.numpy() - ref.running_mean).max() <= 1e-12 * scale, case.name
            assert np.abs(mod.running_var.numpy() - ref.running_var).max() <= 1e-12 * scale, case.name
            assert int(mod.num_batches_tracked) == 1


def test_float32_restatement_sits_within_half_of_every_bound():
    worst = {}
    for case in _all_cases():
        ref = bn.reference(case)
        bn.merge(worst, bn.check(case, ref, bn.restate32(case), limit=0.5))
    print("float32 restatement, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert set(worst) == {"save_mean", "save_rstd", "running_mean", "running_var", "y", "grad_x", "grad_beta", "grad_gamma"}


def test_elements_on_the_relu_gate_are_rare_in_every_case():
    worst = 0.0
    for case in _all_cases():
        ref = bn.reference(case)
        share = float(ref.excluded.mean())
        worst = max(worst, share)
        assert share <= bn.EXCLUDED_CAP, (case.name, share)
    print(f"largest share of gate elements: {worst:.2e}")


def test_case_lists_hold_what_they_claim():
    shapes = bn.shape_cases()
    assert {c.x.shape[0] for c in shapes} == {1, 2, 15, 16, 17, 33, 4080, 4081, 4097, 8209}
    assert {c.x.shape[1] for c in shapes} == {1, 3, 4, 64, 65, 68, 255, 256, 260}
    assert len(bn.PAIRS) == 20 and any(c.p == 1.0 for c in shapes) and any(c.no_running for c in shapes)
    for case in bn.off_centre_cases():
        x = case.x.astype(np.float64)
        assert x[:, -1].std() == 0.0 and abs(abs(x[:, 4].mean()) - 1000.0) < 1.0 and 0.8 < x[:, 4].std() < 1.2
    assert {c.misalign for c in bn.misaligned_cases()} == {None, "x", "gamma", "save_mean"}
    ext = bn.extent_cases()
    assert {(c.x.shape[0], c.rows) for c in ext} == {(4097, 1), (4097, 16), (4097, 17), (4097, 4096), (4097, 4097), (33, 20)}
    assert any(c.seed_dev for c in ext) and all(np.isnan(c.x[c.rows:]).all() for c in ext)
    for case in bn.external_cases():
        pa, pb = bn.external_partials(case)
        live = (case.m + case.ext_rows_per_part - 1) // case.ext_rows_per_part
        assert pa.shape[0] * case.ext_rows_per_part >= case.x.shape[0] and np.isfinite(pa[:live]).all() and np.isnan(pa[live:]).all()
        x = case.x[:case.m].astype(np.float64)
        assert np.allclose(pa[:live].sum(axis=0), x.sum(axis=0), rtol=1e-13) and np.allclose(pb[:live].sum(axis=0), (x * x).sum(axis=0), rtol=1e-13)
    assert max(bn.external_partials(c)[0].shape[0] for c in bn.external_cases()) == 625


def test_mask_restatement_keep_rate_and_seed_words():
    for p in (0.1, 0.5, 0.9):
        keep = bn.keep_mask(1234, 4096, 256, p)                        # ~1 M draws: sigma < 5e-4
        assert abs(float(keep.mean()) - (1 - p)) < 0.003
        assert float(np.abs(keep.mean(axis=0) - (1 - p)).max()) < 0.04 and float(np.abs(keep.mean(axis=1) - (1 - p)).max()) < 0.17
    assert bn.keep_mask(7, 64, 64, 0.0).all() and not bn.keep_mask(7, 64, 64, 1.0).any()
    assert bn.drop_threshold(0.5) == 1 << 23 and bn.drop_threshold(np.float32(0.1)) == int(float(np.float32(0.1)) * 2 ** 24)
    a, b = bn.keep_mask(5, 512, 64, 0.5), bn.keep_mask(5 + (1 << 32), 512, 64, 0.5)       # seeds that differ only in the high word
    assert 0.4 < float((a != b).mean()) < 0.6
    assert np.array_equal(bn.keep_mask(5, 64, 64, 0.5, seed_dev=(1 << 64) - 2), bn.keep_mask(3, 64, 64, 0.5))      # the sum wraps at 2^64
    assert np.array_equal(bn.keep_mask(9, 40, 64, 0.5)[:17], bn.keep_mask(9, 17, 64, 0.5))  # an extent does not change the index
