"""The row L2 normalisation without a GPU: the float64 reference, the rounding bounds and the special rows of tests/l2norm_cases.py proved
on the CPU (a float32 restatement inside the bounds, wrong restatements outside them, torch.nn.functional.normalize and its autograd
gradient inside them), and the host side of the three entry points: exports, refusals, and the SAGEConv constructor they complete."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import l2norm_cases as cases
from conftest import ROOT

NEW_SYMBOLS = ("sage_l2_normalize_forward", "sage_l2_normalize_backward", "sage_l2_normalize_kernel_name_at")


# ------------------------------------------------------------------------------------------------ reference and bounds

def test_cases_cover_the_table_and_keep_the_bounds_premises():
    assert {(c.m, c.c) for c in cases.GRID} >= {(m, c) for m in (1, 3, 255, 257) for c in (1, 3, 7, 63, 64, 65, 256, 300)}
    assert {c.c % 4 for c in cases.GRID} == {0, 1, 2, 3} and {c.c % 4 for c in cases.SPECIAL} == {0, 3}
    tiny = float(np.finfo(np.float32).tiny)
    for case in cases.CASES:
        x, g = cases.inputs(case)
        ref, clamped, bound = cases.expectation(case)
        live = cases.live_rows(case)
        norms = np.sqrt((x.astype(np.float64) ** 2).sum(1))[live]
        assert not ((norms > cases.EPS * (1 - 2.0 ** -10)) & (norms < cases.EPS * (1 + 2.0 ** -10))).any(), case.id
        for t in (ref.y, ref.inv, ref.gx):
            v = np.abs(t[live])
            assert np.isfinite(v).all() and not ((v > 0) & (v < tiny)).any(), case.id            # nothing subnormal
        open_rows = live & ~clamped
        sq = (x.astype(np.float64) ** 2)[open_rows]
        assert sq.size == 0 or sq.min() > 1e3 * tiny, case.id                                   # the squares stay clear of underflow
        if case.group == "special":
            assert clamped[1] and clamped[3] and int(clamped[live].sum()) == 2
            assert set(np.flatnonzero(~live)) == {5, 7, 9}
        else:
            assert not clamped.any()
            if case.m >= 3:                                                                      # a row eps-on-the-square would clamp
                assert ((norms > 1e-12) & (norms < 1e-6)).any(), case.id


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.id)
def test_float32_restatement_is_inside_the_bounds(case):
    got = cases.restate32(*cases.inputs(case))
    print(case.id, "worst error / bound", cases.worst_ratio(case, got))
    assert cases.violations(case, got) == {"y": 0, "inv": 0, "gx": 0}


@pytest.mark.parametrize("wrong", cases.WRONG)
@pytest.mark.parametrize("group", cases.GROUPS)
def test_wrong_restatements_are_outside_the_bounds(group, wrong):
    """Each mistake shows on at least one case of every group, in the quantity it touches."""
    caught = {}
    for case in cases.CASES:
        if case.group == group:
            v = cases.violations(case, cases.restate32(*cases.inputs(case), wrong=wrong))
            caught[case.id] = v["gx"] if wrong == "no_projection" else v["y"] + v["inv"]
    assert any(caught.values()), (group, wrong, caught)
    if wrong == "no_projection":                          # ... and this one on every case wider than one column
        assert all(n > 0 for k, n in caught.items() if not k.endswith("x1")), caught


def _torch_result(x, g):
    xt = torch.from_numpy(np.array(x)).requires_grad_(True)
    y = F.normalize(xt, p=2.0, dim=-1, eps=1e-12)
    y.backward(torch.from_numpy(np.array(g)))
    inv = 1.0 / torch.linalg.vector_norm(xt.detach(), dim=-1).clamp_min(1e-12)
    return cases.Result(y.detach().numpy(), inv.numpy(), xt.grad.numpy())


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.id)
def test_torch_normalize_is_inside_the_bounds(case):
    """F.normalize and its autograd gradient on the CPU, float32: what the kernels replace meets the same bounds against the same float64
    reference, the clamp branch included."""
    got = _torch_result(*cases.inputs(case))
    print(case.id, "worst error / bound", cases.worst_ratio(case, got))
    assert cases.violations(case, got) == {"y": 0, "inv": 0, "gx": 0}


@pytest.mark.parametrize("case", cases.SPECIAL, ids=lambda c: c.id)
def test_special_rows_are_what_torch_and_the_restatement_give(case):
    """The exactly stated rows: the float32 restatement gives them value for value, and so does torch -- up to the one product x * (1 / eps)
    where torch divides (below_eps: inside the bound, checked above) and the NaN pattern of the inf row's gradient, which torch's
    formula spreads differently (the row is NaN there too wherever the rule's is not zero)."""
    x, g = cases.inputs(case)
    want = cases.special_expectation(case)
    mine, theirs = cases.restate32(x, g), _torch_result(x, g)
    for row, kind in cases.SPECIAL_ROWS.items():
        w = want[row]
        assert cases.same_values(mine.y[row], w.y) and cases.same_values(mine.inv[row], w.inv) and cases.same_values(mine.gx[row], w.gx), kind
        if kind in ("zero", "nan", "overflow"):
            assert cases.same_values(theirs.y[row], w.y) and cases.same_values(theirs.gx[row], w.gx), kind
        if kind == "zero":
            assert cases.same_values(theirs.gx[row], g[row] / np.float32(cases.EPS))
        if kind == "inf":
            assert cases.same_values(theirs.y[row], w.y) and np.isnan(theirs.gx[row]).any()
        if kind == "overflow":                                              # torch's own float32 result for the row: zeros
            assert not theirs.y[row].any() and not theirs.gx[row].any()
    rest = [r for r in range(case.m) if r not in cases.SPECIAL_ROWS]         # the neighbours: finite, unit norm
    assert np.isfinite(mine.y[rest]).all() and np.isfinite(mine.gx[rest]).all()
    assert np.allclose(np.linalg.norm(mine.y[rest].astype(np.float64), axis=1), 1.0, atol=1e-5)


# ------------------------------------------------------------------------------------------------ the ABI

@pytest.fixture(scope="module")
def lib():
    from graphpope_amd import _lib
    return _lib.load()


def test_new_symbols_are_exported_and_declared(lib):
    from graphpope_amd import _lib
    header = open(os.path.join(ROOT, "include", "graphpope_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    for name, n_args in zip(NEW_SYMBOLS, (8, 9, 5)):
        decl = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == n_args, name
    assert "torch.nn.functional.normalize(x, p=2, dim=-1, eps=1e-12)" in header


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Null matrices, C = 0, M < 0, M >= 2^31 - 1 and eps <= 0: POPE_ERR_INVALID with the entry point named in the error string.  The
    pointers handed over are host arrays, so a launch would not go unnoticed; M = 0 is fine and launches nothing."""
    from graphpope_amd import _lib
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    eps = cases.EPS

    def fwd(x, m, c, e, y, inv):
        return lib.sage_l2_normalize_forward(x, m, c, e, y, inv, null, null)

    def bwd(y, inv, g, m, c, e, gx):
        return lib.sage_l2_normalize_backward(y, inv, g, m, c, e, gx, null, null)

    for bad in ((null, 4, 4, eps, p, p), (p, 4, 4, eps, null, p), (p, 4, 4, eps, p, null), (p, 4, 0, eps, p, p), (p, -1, 4, eps, p, p),
                (p, 2 ** 31 - 1, 4, eps, p, p), (p, 4, 4, 0.0, p, p)):
        assert fwd(*bad) == _lib.ERR_INVALID, bad
        assert b"sage_l2_normalize_forward" in lib.pope_last_error()
    for bad in ((null, p, p, 4, 4, eps, p), (p, null, p, 4, 4, eps, p), (p, p, null, 4, 4, eps, p), (p, p, p, 4, 4, eps, null),
                (p, p, p, 4, 0, eps, p), (p, p, p, -1, 4, eps, p), (p, p, p, 2 ** 31 - 1, 4, eps, p), (p, p, p, 4, 4, -1.0, p)):
        assert bwd(*bad) == _lib.ERR_INVALID, bad
        assert b"sage_l2_normalize_backward" in lib.pope_last_error()
    assert fwd(p, 0, 4, eps, p, p) == _lib.OK and bwd(p, p, p, 0, 4, eps, p) == _lib.OK and lib.pope_last_error() == b""
    assert all(v == 0.0 for v in buf)


def test_kernel_name_query_follows_width_and_alignment(lib):
    from graphpope_amd import _lib
    buf = ctypes.create_string_buffer(96)

    def name(m, c, mask):
        _lib.check(lib.sage_l2_normalize_kernel_name_at(m, c, mask, buf, 96))
        return buf.value.decode()

    both = "k_l2_normalize<%s>+k_l2_normalize_backward<%s>"
    assert name(257, 256, 0) == both % ("true", "true") and name(1, 4, 0) == both % ("true", "true")
    for c in (1, 3, 7, 63, 65):
        assert name(257, c, 0) == both % ("false", "false")
    assert name(257, 256, 1) == both % ("false", "true")               # x: the forward call alone
    assert name(257, 256, 2) == both % ("false", "false")              # y: both read it
    assert name(257, 256, 4) == name(257, 256, 8) == both % ("true", "false")
    assert lib.sage_l2_normalize_kernel_name_at(257, 256, 16, buf, 96) == _lib.ERR_INVALID
    assert lib.sage_l2_normalize_kernel_name_at(0, 256, 0, buf, 96) == _lib.ERR_INVALID
    assert lib.sage_l2_normalize_kernel_name_at(257, 0, 0, buf, 96) == _lib.ERR_INVALID
    assert lib.sage_l2_normalize_kernel_name_at(257, 256, 0, None, 96) == _lib.ERR_INVALID
    assert name(3, 300, 0) == both % ("true", "true") and lib.pope_last_error() == b""                 # (clears the error string)


# ------------------------------------------------------------------------------------------------ the constructor

def test_sageconv_takes_pyg_signature():
    from graphpope_amd import sage
    conv = sage.SAGEConv(8, 8, normalize=True)
    assert conv.normalize and sorted(conv.state_dict()) == ["lin_l.bias", "lin_l.weight", "lin_r.weight"]
    positional = sage.SAGEConv(8, 6, True, True, False)                 # (in, out, normalize, root_weight, bias): PyG 1.7.0's order
    assert positional.normalize and positional.lin_l.bias is None
    assert not sage.SAGEConv(8, 8).normalize and sage.SAGEConv(8, 8).lin_l.bias is not None


def test_sageconv_without_bias_has_no_bias_in_its_state_dict():
    from graphpope_amd import sage
    conv = sage.SAGEConv(8, 8, bias=False)
    assert sorted(conv.state_dict()) == ["lin_l.weight", "lin_r.weight"] and [k for k, _ in conv.named_parameters()] == ["lin_l.weight", "lin_r.weight"]


def test_sageconv_without_root_weight_is_refused():
    from graphpope_amd import sage
    with pytest.raises(NotImplementedError, match="root_weight"):
        sage.SAGEConv(8, 8, root_weight=False)


def test_sage_passes_normalize_to_every_conv():
    from graphpope_amd import sage
    assert all(c.normalize for c in sage.SAGE(12, 5, 16, 3, normalize=True).convs)
    assert not any(c.normalize for c in sage.SAGE(12, 5, 16, 3).convs)
    torch.manual_seed(4)
    a = sage.SAGE(12, 5, 16, 3)
    torch.manual_seed(4)
    b = sage.SAGE(12, 5, 16, 3, dropout=0.5, normalize=False)
    assert sorted(a.state_dict()) == sorted(b.state_dict()) and all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
