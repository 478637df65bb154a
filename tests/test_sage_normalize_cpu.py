"""tests/sage_normalize_cases.py proved on the CPU: the float64 references of the normalising conv and of the two-layer model, their
thresholds, and the two shortcuts a normalising conv must not take -- restated, they fall outside the thresholds."""
import numpy as np
import pytest
import torch

import sage_model_cases as mc
import sage_normalize_cases as cases


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("c_out", cases.C_OUTS)
def test_conv_reference_and_threshold(c_out, bias):
    t, blk = cases.conv_inputs(c_out, bias)
    rowptr, col = blk
    assert rowptr[cases.EMPTY_ROW + 1] == rowptr[cases.EMPTY_ROW] and len(rowptr) - 1 == cases.N_DST and col.max() < cases.N_SRC
    ref, limit = cases.conv_yardstick(t, blk)
    assert set(ref) == {"out", "grad:x", "grad:w_l", "grad:w_r"} | ({"grad:b_l"} if bias else set())
    assert torch.allclose(ref["out"].norm(dim=1), torch.ones(cases.N_DST, dtype=torch.float64), atol=1e-12)       # every row, the empty one too
    assert cases.conv_check(cases.run_conv(t, blk, torch.float32, perm=2), ref, limit, "restatement") <= 1.0
    # the same conv without the normalisation is far outside: output and every gradient
    plain = cases.run_conv(t, blk, torch.float32, normalize=False)
    assert all(cases.err(plain[k], ref[k]) > 100 * limit[k] for k in ref)
    # the dense formulation against the edge-list one of the model reference
    a = cases.dense_mean(rowptr, col, cases.N_SRC, torch.float64)
    assert torch.allclose(a.sum(1), torch.tensor(np.diff(rowptr) > 0, dtype=torch.float64))


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_model_reference_threshold_and_the_two_shortcuts(p):
    seeds = mc.drawn_seeds(cases.MANUAL_SEED, 1) if p > 0 else [0]
    inp = cases.model_inputs(p, seeds)
    yard = cases.yardstick(inp)
    assert yard.gated == [0] and yard.elements == [40 * 16]                                     # no element near the ReLU's kink
    assert set(yard.scale) == {"logits", "y.0", "running_mean.0", "running_var.0", "grad:bns.0.weight", "grad:bns.0.bias"} | {
        "grad:convs.%d.%s" % (i, k) for i in (0, 1) for k in ("lin_l.weight", "lin_l.bias", "lin_r.weight")}
    keep = inp.keeps[0]
    assert bool(keep.all()) == (p == 0.0) and (p == 0.0 or 0.3 < float(keep.float().mean()) < 0.7)
    # the restatement in an order of its own is inside
    rep = mc.check(yard, cases.run_model(inp, torch.float32, patterns=yard.ref.patterns, perm=4).out, "restatement")
    assert rep["worst"] <= 1.0
    # the logits are unit rows: the last conv normalises too
    assert torch.allclose(yard.ref.out["logits"].norm(dim=1), torch.ones(16, dtype=torch.float64), atol=1e-12)
    # statistics of the un-normalised projection: the hidden activations (and what follows) leave the bound
    rep = mc.check(yard, cases.run_model(inp, torch.float32, patterns=yard.ref.patterns, wrong="shortcut_stats").out, "shortcut_stats", must_hold=False)
    assert rep["tensors"]["y.0"]["ratio"] > 10 and rep["tensors"]["running_var.0"]["ratio"] > 10, rep["tensors"]
    # the bias gradient as column sums of the gradient behind the normalisation: only that tensor moves, and it leaves the bound
    rep = mc.check(yard, cases.run_model(inp, torch.float32, patterns=yard.ref.patterns, wrong="shortcut_bias").out, "shortcut_bias", must_hold=False)
    assert rep["tensors"]["grad:convs.0.lin_l.bias"]["ratio"] > 10, rep["tensors"]
    assert all(v["ratio"] <= 1.0 for k, v in rep["tensors"].items() if k != "grad:convs.0.lin_l.bias")


def test_model_reference_without_normalisation_is_the_existing_one():
    """normalize=False: this file's model is sage_model_cases.run_model, tensor for tensor."""
    inp = cases.model_inputs(0.5, mc.drawn_seeds(cases.MANUAL_SEED, 1))
    mine = cases.run_model(inp, torch.float64, normalize=False)
    theirs = mc.run_model(inp, torch.float64)
    assert set(mine.out) == set(theirs.out)
    for k in mine.out:
        assert torch.allclose(mine.out[k], theirs.out[k], rtol=1e-12, atol=1e-14), k


def test_conv_bn_reference_and_the_two_shortcuts_at_the_handoff_shape():
    """The shape whose plain projection hands BatchNorm its statistics: the restatement is inside the threshold, both shortcuts outside."""
    t, blk = cases.conv_bn_inputs()
    ref, limit, gated, _ = cases.conv_bn_yardstick(t, blk)
    _, _, pattern = cases.run_conv_bn(t, blk, torch.float64)
    assert gated <= 1e-3 * ref["out"].numel()
    assert set(ref) == {"out", "grad:x", "grad:w_l", "grad:b_l", "grad:w_r", "grad:gamma", "grad:beta"}
    inside, _, _ = cases.run_conv_bn(t, blk, torch.float32, pattern=pattern, perm=3)
    assert cases.conv_check(inside, ref, limit, "restatement") <= 1.0
    stats, _, _ = cases.run_conv_bn(t, blk, torch.float32, pattern=pattern, wrong="shortcut_stats")
    assert cases.err(stats["out"], ref["out"]) > 10 * limit["out"]
    bias, _, _ = cases.run_conv_bn(t, blk, torch.float32, pattern=pattern, wrong="shortcut_bias")
    assert cases.err(bias["grad:b_l"], ref["grad:b_l"]) > 10 * limit["grad:b_l"]
    assert all(cases.err(bias[k], ref[k]) <= limit[k] for k in ref if k != "grad:b_l")


@pytest.mark.parametrize("num_layers, hops", [(2, 2), (3, 2), (3, 3)])
def test_eval_reference_and_threshold(num_layers, hops):
    state = cases.eval_model(num_layers).state_dict()
    ref, limit = cases.eval_yardstick(state, hops)
    assert ref.shape == (cases.EVAL_N, 5 if hops == num_layers else 16)
    assert torch.allclose(ref.norm(dim=1), torch.ones(cases.EVAL_N, dtype=torch.float64), atol=1e-12)
    assert cases.err(cases.run_eval(state, hops, torch.float32, perm=2), ref) <= limit < 1e-4
    plain = cases.eval_model(num_layers, normalize=False)
    assert sorted(plain.state_dict()) == sorted(state)
