"""GATv2Conv / GATv2 without a GPU, through tests/gatv2_cases.py: the dense float64 reference against the edge form, the gate shares,
the restatement of e against a plain float64 dot, and everything of pope_gatv2_* and graphpope_amd/gatv2.py that is host logic --
the symbols, argument checks of every entry point, the size and name queries, the constructors, the refusals, and the
GRAPHPOPE_GCN_LAYER=gatv2 switch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gatv2_cases as cases
from conftest import ROOT

SYMBOLS = ("pope_gatv2_scores", "pope_gatv2_attention", "pope_gatv2_conv_forward_scratch_size", "pope_gatv2_conv_forward",
           "pope_gatv2_conv_backward_scratch_size", "pope_gatv2_conv_backward", "pope_gatv2_kernel_name")


@pytest.fixture(scope="module")
def lib():
    from graphpope_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _leave_no_error_string_behind(lib):
    """The refusals tested here set pope_last_error; a successful query clears it, so that no later test of the process finds it."""
    yield
    buf = ctypes.create_string_buffer(1536)
    assert lib.pope_gatv2_kernel_name(1, 0, 4, 1, 4, 1, 0, 0, 1, 256, 0, buf, 1536) == 0 and lib.pope_last_error() == b""


def p(v):
    return ctypes.c_void_p(v)


FAKE = 4096                       # a pointer that is never dereferenced: validation happens before anything touches the device


# ------------------------------------------------------------------------------------------------ the reference side

@pytest.mark.parametrize("case", cases.LAYER_CASES, ids=lambda c: c.id)
def test_dense_reference_is_the_edge_form_and_the_gate_share_stays_under_the_cap(case):
    """The edge form in float64 IS the dense reference (to ~1e-12); the float32 restatements sit near float32 rounding relative to the
    conditioning of the case; the reference alone keeps the gated share under the cap."""
    share = cases.gate_share(case)
    print(case.id, "gated share", share)
    assert share <= cases.EXCLUDED_CAP
    t64, err32, _, mismatches = cases.layer_expectation(case)
    assert mismatches is None
    assert set(err32) == {"out", "grad_x"} | {"grad_" + k for k in case.param_keys}
    bound = 2.0 ** -10 if case.att_scale != 1.0 else 2.0 ** -16
    for k, e in err32.items():
        assert 0 < e < bound, (k, e)
    conf = cases._conf(case)
    again = cases._layer_tensors(case, lambda x, q: cases.edge_layer(case.graph, x, q, *conf, 3), torch.float64)
    for k in t64:
        print(case.id, k, cases.err(again[k], t64[k]))
        assert cases.err(again[k], t64[k]) < 1e-12, k
        assert bool(torch.isfinite(t64[k]).all())


def test_the_overflow_case_overflows_without_the_max_subtraction():
    case = cases.OVERFLOW_CASE
    t = {k: torch.from_numpy(v).double() for k, v in cases.layer_inputs(case).items()}
    hl, hr = cases._project(t["x"], {k: t[k] for k in case.param_keys}, case.H, case.C)
    src, dst = cases.gc._edges(case.graph, True, None)
    z = hl[src] + hr[dst]
    e = (torch.where(z > 0, z, 0.2 * z) * t["att"]).sum(-1)
    with np.errstate(over="ignore"):
        assert float(e.abs().max()) > 150.0 and not np.isfinite(np.exp(np.float32(e.abs().max())))


@pytest.mark.parametrize("case", (cases.LAYER_CASES[1], cases.LAYER_CASES[12]), ids=lambda c: c.id)
def test_rows_of_the_reference_alpha_sum_to_one_or_to_zero(case):
    g = cases.graph("main")
    alpha, alpha_self = cases.reference_alpha(case)
    rowptr, col = cases.canonical("main", False)
    rows = torch.from_numpy(np.repeat(np.arange(g.n), np.diff(rowptr)).astype(np.int64))
    total = torch.zeros((g.n, case.H), dtype=torch.float64).index_add_(0, rows, alpha) + alpha_self
    has_terms = torch.ones(g.n, dtype=torch.bool) if case.add_self_loops else torch.from_numpy(np.diff(rowptr) > 0)
    assert bool((~has_terms).any()) == (not case.add_self_loops)
    assert float((total[has_terms] - 1).abs().max()) < 1e-12 and float(total[~has_terms].abs().sum()) == 0.0


@pytest.mark.parametrize("H,C", [s[1:] for s in cases.SHAPES])
def test_e_restatement_against_a_plain_float64_dot(H, C):
    """The documented order is a sum of the same H C products: it differs from the float64 dot by float32 rounding of at most
    C + 2 operations per head (products, the adds of the fold), relative to sum |att leaky(z)|."""
    g = cases.graph("main")
    rs = np.random.RandomState(300 + 7 * H + C)
    hl, hr = (0.25 + rs.randn(g.n, H, C)).astype(np.float32), rs.randn(g.n, H, C).astype(np.float32)
    att = (rs.randn(H, C) / np.sqrt(C)).astype(np.float32)
    src, dst = rs.randint(0, g.n, size=500), rs.randint(0, g.n, size=500)
    got = cases.e_restatement(hl, hr, att, src, dst, 0.2)
    z = hl[src].astype(np.float32) + hr[dst].astype(np.float32)              # the float32 sum is part of the definition
    terms = att[None].astype(np.float64) * np.where(z > 0, z, np.float32(0.2) * z).astype(np.float64)
    want, scale = terms.sum(-1), np.abs(terms).sum(-1)
    assert got.dtype == np.float32 and got.shape == (500, H)
    assert (np.abs(got - want) <= (C + 2) * 2.0 ** -24 * scale + 1e-30).all()
    dot = cases.dot_restatement(hr, hl, src, dst)
    want = (hr[dst].astype(np.float64) * hl[src].astype(np.float64)).sum(-1)
    assert (np.abs(dot - want) <= (C + 2) * 2.0 ** -24 * (np.abs(hr[dst].astype(np.float64) * hl[src]).sum(-1)) + 1e-30).all()


def test_model_reference_gate_and_restatements():
    ref, err32, share, mismatches = cases.model_expectation()
    assert mismatches is None and share <= cases.EXCLUDED_CAP
    assert set(err32) == {"logits"} | {"grad:" + k for k in cases.PARAMS}
    for k, e in err32.items():
        assert 0 < e < 2.0 ** -16, (k, e)
    assert np.isfinite(ref["loss"])


# ------------------------------------------------------------------------------------------------ host logic of the library

def test_every_new_symbol_is_in_the_header_the_signatures_and_the_library(lib):
    from graphpope_amd import _lib
    with open(os.path.join(ROOT, "include", "graphpope_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert sorted(k for k in _lib.SIGNATURES if k.startswith("pope_gatv2_")) == sorted(SYMBOLS)


def test_argument_checks_of_every_entry_point(lib):
    from graphpope_amd import _lib
    f = p(FAKE)
    ok = dict(N=10, nnz=20, c_in=4, H=2, C=4, slope=0.2)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.pope_gatv2_conv_forward(f, f, a["N"], a["nnz"], f, a["c_in"], f, None, kw.get("w_r", f), None, f, None, a["H"], a["C"], 1,
                                           a["slope"], 1, p(12288), kw.get("hr", p(8192)), p(16384), p(20480), f, kw.get("scratch", f), kw.get("bytes", 0), None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.pope_gatv2_conv_backward(f, f, f, f, f, a["N"], a["nnz"], f, a["c_in"], f, kw.get("w_r", f), f, a["H"], a["C"], 1, a["slope"], 1,
                                            f, kw.get("hr", f), f, f, f, None, f, None, kw.get("gw_r", f), None, f, None, kw.get("scratch", f),
                                            kw.get("bytes", 0), None)

    def scores(**kw):
        a = dict(ok, **kw)
        return lib.pope_gatv2_scores(f, f, a["N"], a["nnz"], f, kw.get("hr", f), a["H"], a["C"], f, a["slope"], 1, f, f, None)

    def attention(**kw):
        a = dict(ok, **kw)
        return lib.pope_gatv2_attention(f, f, a["N"], a["nnz"], f, kw.get("hr", f), a["H"], a["C"], f, a["slope"], 1, f, f, f, kw.get("alpha_self", f),
                                        None)

    bad = (dict(N=0), dict(N=2 ** 31 - 1), dict(nnz=-1), dict(nnz=2 ** 31 - 1), dict(H=0), dict(C=0), dict(H=2 ** 15, C=2 ** 15),
           dict(slope=-0.1), dict(slope=1.5), dict(slope=float("nan")), dict(hr=None))
    for kw in bad:
        for call, name in ((fwd, b"pope_gatv2_conv_forward"), (bwd, b"pope_gatv2_conv_backward"), (scores, b"pope_gatv2_scores"),
                           (attention, b"pope_gatv2_attention")):
            assert call(**kw) == _lib.ERR_INVALID and name in lib.pope_last_error(), (kw, name)
    for kw in (dict(c_in=0), dict(scratch=None)):
        assert fwd(**kw) == _lib.ERR_INVALID and bwd(**kw) == _lib.ERR_INVALID, kw
    assert fwd(slope=2.0) == _lib.ERR_INVALID and b"negative_slope" in lib.pope_last_error()
    assert fwd(hr=p(12288)) == _lib.ERR_INVALID and b"hr must not alias hl" in lib.pope_last_error()
    for k, which in enumerate(("hl", "hr", "alpha", "alpha_self")):           # out aliasing a tensor the propagate reads
        ptrs = [p(4096 + 4096 * (i + 1)) for i in range(4)]
        rc = lib.pope_gatv2_conv_forward(f, f, 10, 20, f, 4, f, None, f, None, f, None, 2, 4, 1, 0.2, 1, *ptrs, ptrs[k], f, 1 << 20, None)
        assert rc == _lib.ERR_INVALID and b"out must not alias" in lib.pope_last_error(), which
    assert bwd(gw_r=None) == _lib.ERR_INVALID and attention(alpha_self=None) == _lib.ERR_INVALID
    # a short scratch: refused with the needed size, before anything is launched; shared weights need neither hr nor grad_weight_r
    need = lib.pope_gatv2_conv_forward_scratch_size(10, 20, 4, 2, 4, 1)
    assert fwd(bytes=need - 1) == _lib.ERR_WORKSPACE and str(need).encode() in lib.pope_last_error()
    assert fwd(bytes=need - 1, w_r=None, hr=None) == _lib.ERR_WORKSPACE
    need = lib.pope_gatv2_conv_backward_scratch_size(10, 20, 4, 2, 4, 1)
    assert bwd(bytes=need - 1) == _lib.ERR_WORKSPACE and str(need).encode() in lib.pope_last_error()
    assert bwd(bytes=need - 1, w_r=None, hr=None, gw_r=None) == _lib.ERR_WORKSPACE


def test_size_queries(lib):
    n, nnz = 89250, 899756
    queries = (lib.pope_gatv2_conv_forward_scratch_size, lib.pope_gatv2_conv_backward_scratch_size)
    for q in queries:
        assert q(0, nnz, 8, 8, 32, 1) == 0 and q(n, -1, 8, 8, 32, 1) == 0 and q(n, nnz, 0, 8, 32, 1) == 0 and q(n, nnz, 8, 0, 32, 1) == 0
        assert q(n, nnz, 8, 8, 0, 1) == 0 and q(n, nnz, 8, 2 ** 15, 2 ** 15, 1) == 0 and q(2 ** 31 - 1, nnz, 8, 8, 32, 1) == 0
        assert q(n, 2 ** 31 - 1, 8, 8, 32, 1) == 0
        base = q(n, nnz, 8, 8, 32, 1)
        assert base > 0 and base % 256 == 0
        for doubled in ((2 * n, nnz, 8, 8, 32), (n, 2 * nnz, 8, 8, 32), (n, nnz, 16, 8, 32), (n, nnz, 8, 16, 32), (n, nnz, 8, 8, 64)):
            assert q(*doubled, 1) >= base, doubled
            assert q(*doubled, 0) >= q(*doubled, 1)
    assert lib.pope_gatv2_conv_forward_scratch_size(n, nnz, 500, 8, 32, 1) == lib.pope_gat_conv_forward_scratch_size(n, nnz, 500, 8, 32, 1)
    back = lib.pope_gatv2_conv_backward_scratch_size(n, nnz, 500, 8, 32, 1)
    assert back >= nnz * 8 * 4 + 3 * n * 256 * 4 + n * 8 * 4
    assert lib.pope_gatv2_conv_backward_scratch_size(n, nnz, 500, 8, 32, 0) - back == n * 256 * 4      # the spread gradient


def test_kernel_names_follow_the_shapes(lib):
    buf = ctypes.create_string_buffer(1536)

    def name(n, nnz, c_in, H, C, concat=1, share=0, backward=0, grad_x=1, mis=0, cap=1536):
        from graphpope_amd import _lib
        _lib.check(lib.pope_gatv2_kernel_name(n, nnz, c_in, H, C, concat, share, backward, grad_x, cases.CUS, mis, buf, cap))
        return buf.value.decode().split("+")

    g = cases.graph("main")
    fwd = name(g.n, g.nnz, 36, 4, 64)
    assert fwd[0].startswith("k_gemm<") and fwd[1].startswith("k_gemm<")
    assert fwd[2:] == ["k_gatv2_scores<true, true, false, true>", "k_gatv2_softmax", "k_gcn_clear", "k_gat_propagate<true, false>",
                       "k_gat_hub_partial<true, false>", "k_gat_hub_finish<true, false>"]
    shared = name(g.n, g.nnz, 36, 4, 64, share=1)
    assert shared == fwd[1:]
    assert name(g.n, g.nnz, 36, 4, 64, concat=0)[-1] == "k_gat_head_mean"
    assert "k_gatv2_scores<false, false, false, true>" in name(g.n, g.nnz, 12, 3, 7) and "k_gatv2_scores<true, false, false, false>" in name(g.n, g.nnz, 36, 2, 130)
    assert "k_gatv2_scores<true, true, false, false>" in name(g.n, g.nnz, 12, 1, 260) and "k_gatv2_scores<true, true, false, false>" in name(g.n, g.nnz, 12, 3, 100)
    for bit in (3, 4, 5):                                                                   # hl, hr, att off the 16-byte grid
        assert "k_gatv2_scores<false, true, false, true>" in name(g.n, g.nnz, 36, 4, 64, mis=1 << bit)
    assert "k_gatv2_scores<true, true, false, true>" in name(g.n, g.nnz, 36, 4, 64, share=1, mis=1 << 4)      # shared weights: hr is hl
    assert name(89250, 899756, 500, 8, 32)[0].startswith("k_gemm_tile16<")
    bwd = name(g.n, g.nnz, 36, 4, 64, backward=1)
    assert bwd[:2] == ["k_gatv2_scores<true, true, true, true>", "k_gatv2_edge_grad"]
    assert bwd[2:6] == ["k_gcn_clear", "k_gatv2_rowsum<true, false>", "k_gatv2_hub_partial<true, false>", "k_gatv2_hub_finish<true, false>"]
    assert bwd[6:10] == ["k_gcn_clear", "k_gatv2_rowsum<true, true>", "k_gatv2_hub_partial<true, true>", "k_gatv2_hub_finish<true, true>"]
    assert bwd[10:12] == ["k_colsum_partial<true>", "k_colsum_final"] and "[splits=" in bwd[12] and bwd[13] == "k_slab_reduce"
    assert bwd[-3].startswith("k_gemm<") and bwd[-2:] == ["k_colsum_partial<true>", "k_colsum_final"]
    assert len(name(g.n, g.nnz, 36, 4, 64, backward=1, grad_x=0)) == len(bwd) - 1
    assert "k_gatv2_add" in name(g.n, g.nnz, 36, 4, 64, share=1, backward=1) and "k_gatv2_add" not in bwd
    assert name(g.n, g.nnz, 36, 4, 64, concat=0, backward=1)[0] == "k_gat_spread_grad"
    assert "k_gcn_clear" not in name(17, 0, 36, 4, 64, backward=1)
    assert lib.pope_gatv2_kernel_name(0, 5, 4, 1, 4, 1, 0, 0, 1, 256, 0, buf, 1536) != 0
    assert lib.pope_gatv2_kernel_name(5, 5, 4, 1, 4, 1, 0, 0, 1, 256, 1 << 9, buf, 1536) != 0
    assert lib.pope_gatv2_kernel_name(g.n, g.nnz, 36, 4, 64, 1, 0, 1, 1, 256, 0, buf, 16) != 0 and b"do not fit" in lib.pope_last_error()


# ------------------------------------------------------------------------------------------------ the Python layer

def test_constructor_parameters_and_repr():
    from graphpope_amd import gatv2
    conv = gatv2.GATv2Conv(12, 7, heads=3)
    assert sorted(conv.state_dict()) == ["att", "bias", "lin_l.bias", "lin_l.weight", "lin_r.bias", "lin_r.weight"]
    assert conv.lin_l.weight.shape == conv.lin_r.weight.shape == (21, 12) and conv.att.shape == (1, 3, 7) and conv.bias.shape == (21,)
    assert conv.lin_r is not conv.lin_l and conv.lin_l.bias.shape == (21,)
    for b in (conv.bias, conv.lin_l.bias, conv.lin_r.bias):
        assert float(b.detach().abs().sum()) == 0.0
    assert float(conv.lin_l.weight.detach().abs().max()) <= np.sqrt(6.0 / (12 + 21)) and 0 < float(conv.att.detach().abs().max()) <= np.sqrt(6.0 / (3 + 7))
    assert conv.extra_repr() == "12, 7, heads=3" and repr(conv).startswith("GATv2Conv(")
    assert (conv.concat, conv.negative_slope, conv.dropout, conv.add_self_loops, conv.share_weights) == (True, 0.2, 0.0, True, False)
    shared = gatv2.GATv2Conv(12, 7, heads=3, share_weights=True)
    assert sorted(shared.state_dict()) == ["att", "bias", "lin_l.bias", "lin_l.weight"] and shared.lin_r is shared.lin_l
    assert [k for k, _ in shared.named_parameters()] == ["att", "bias", "lin_l.weight", "lin_l.bias"]
    assert shared.extra_repr() == "12, 7, heads=3, share_weights=True"
    mean = gatv2.GATv2Conv(12, 7, heads=3, concat=False, bias=False)
    assert mean.bias is None and mean.lin_l.bias is None and gatv2.GATv2Conv(12, 7, heads=3, concat=False).bias.shape == (7,)
    with pytest.raises(ValueError):
        gatv2.GATv2Conv(12, 7, heads=0)
    with pytest.raises(ValueError, match="negative_slope"):
        gatv2.GATv2Conv(12, 7, negative_slope=1.5)


def test_model_layers_and_hidden_not_a_multiple_of_heads():
    from graphpope_amd import gatv2
    model = gatv2.GATv2(36, 64, 5, num_layers=3, heads=8, dropout=0.5)
    assert [(c.in_channels, c.out_channels, c.heads) for c in model.convs] == [(36, 8, 8), (64, 8, 8), (64, 5, 1)]
    assert all(c.dropout == 0.0 and c.concat for c in model.convs) and model.dropout == 0.5
    assert sorted(model.state_dict()) == sorted(f"convs.{i}.{k}" for i in range(3) for k in cases.PARAM_KEYS)
    assert all(c.share_weights for c in gatv2.GATv2(36, 64, 5, share_weights=True).convs)
    with pytest.raises(ValueError, match="heads"):
        gatv2.GATv2(36, 60, 5, heads=8)
    with pytest.raises(ValueError, match="num_layers"):
        gatv2.GATv2(36, 64, 5, num_layers=0)


def test_attention_dropout_in_training_mode_is_refused_before_the_device_check():
    from graphpope_amd import gatv2
    conv = gatv2.GATv2Conv(4, 4, dropout=0.3)
    conv.train()
    with pytest.raises(NotImplementedError, match="dropout"):
        conv(torch.zeros(3, 4), None)
    conv.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # past the refusal: the layer itself runs on the GPU only
        conv(torch.zeros(3, 4), None)


def test_the_layer_switch_accepts_gatv2_and_keeps_every_refusal(monkeypatch):
    from graphpope_amd import main
    assert main.gcn_layer_from_env(256, {"GRAPHPOPE_GCN_LAYER": "gatv2"}) == ("gatv2", 8)
    assert main.gcn_layer_from_env(60, {"GRAPHPOPE_GCN_LAYER": "gatv2", "GRAPHPOPE_GAT_HEADS": "4"}) == ("gatv2", 4)
    assert main.gcn_layer_from_env(256, {}) == ("gcn", 0) and main.gcn_layer_from_env(256, {"GRAPHPOPE_GCN_LAYER": "gat"}) == ("gat", 8)
    for layer in ("sage", "gatv3", "GATv2", "gatv2 ", ""):
        with pytest.raises(ValueError, match="GRAPHPOPE_GCN_LAYER"):
            main.gcn_layer_from_env(256, {"GRAPHPOPE_GCN_LAYER": layer})
    for heads in ("7", "0", "-2", "many"):
        with pytest.raises(ValueError, match="GRAPHPOPE_GAT_HEADS"):
            main.gcn_layer_from_env(256, {"GRAPHPOPE_GCN_LAYER": "gatv2", "GRAPHPOPE_GAT_HEADS": heads})
    monkeypatch.setenv("GRAPHPOPE_MODEL", "gcn")
    monkeypatch.setenv("GRAPHPOPE_GCN_LAYER", "gatv2")
    monkeypatch.setenv("GRAPHPOPE_GAT_HEADS", "7")
    with pytest.raises(ValueError, match="GRAPHPOPE_GAT_HEADS"):
        main.main(["--dataset", "pubmed", "--epochs", "1", "--hidden_layer_size", "256"])
    monkeypatch.setenv("GRAPHPOPE_GAT_HEADS", "8")
    with pytest.raises(ValueError, match="n_gpus"):                   # --n_gpus > 1 stays refused for the full-batch loop
        main.main(["--dataset", "pubmed", "--epochs", "1", "--n_gpus", "2"])
    monkeypatch.setenv("GRAPHPOPE_MODEL", "gatv2")
    with pytest.raises(ValueError, match="expected sage or gcn"):
        main.model_from_env()
