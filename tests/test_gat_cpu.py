"""GATConv / GAT without a GPU, through tests/gat_cases.py: the restatements against the float64 reference within the rule, the gate
shares, the reference's attention, the slot map's restatement, and everything of pope_gat_* and graphpope_amd/gat.py that is host logic
-- argument checks of every entry point, the size and name queries, the constructors, the refusal of attention dropout, and the
GRAPHPOPE_GCN_LAYER / GRAPHPOPE_GAT_HEADS switches."""
import ctypes

import numpy as np
import pytest
import torch

import gat_cases as cases


@pytest.fixture(scope="module")
def lib():
    from graphpope_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _leave_no_error_string_behind(lib):
    """The refusals tested here set pope_last_error; a successful query clears it, so that no later test of the process finds it."""
    yield
    buf = ctypes.create_string_buffer(768)
    assert lib.pope_gat_kernel_name(1, 0, 4, 1, 4, 1, 0, 1, 256, 0, buf, 768) == 0 and lib.pope_last_error() == b""


def p(v):
    return ctypes.c_void_p(v)


FAKE = 4096                       # a pointer that is never dereferenced: validation happens before anything touches the device


# ------------------------------------------------------------------------------------------------ the reference side

def test_canonical_csrs_hold_the_graph_and_keep_both_hub_edges():
    g = cases.graph("main")
    rowptr, col = cases.canonical("main", False)
    rowptr_t, col_t = cases.canonical("main", True)
    assert np.array_equal(rowptr, g.rowptr) and col.size == col_t.size == g.nnz == 4029
    deg = np.diff(rowptr)
    assert {cases.CHUNK, cases.CHUNK + 1, 2 * cases.CHUNK + 1} <= set(deg.tolist())
    for i in range(g.n):
        assert np.array_equal(col[rowptr[i]:rowptr[i + 1]], np.sort(g.col[g.rowptr[i]:g.rowptr[i + 1]]))
        assert (np.diff(col_t[rowptr_t[i]:rowptr_t[i + 1]]) >= 0).all()


def test_slot_map_restatement_is_a_bijection_that_maps_equal_edges_to_equal_edges():
    g = cases.graph("main")
    rowptr, col = cases.canonical("main", False)
    rowptr_t, col_t = cases.canonical("main", True)
    m = cases.slot_map_restatement("main")
    assert np.array_equal(np.sort(m), np.arange(g.nnz))
    dst_of = np.repeat(np.arange(g.n), np.diff(rowptr))
    src_of_t = np.repeat(np.arange(g.n), np.diff(rowptr_t))
    assert np.array_equal(col[m], src_of_t) and np.array_equal(dst_of[m], col_t)
    pairs = list(zip(src_of_t.tolist(), col_t.tolist()))
    assert len(set(pairs)) < len(pairs)                                 # repeated edges are in it
    for j in range(g.n):                                                # ... and keep their order among themselves
        row = m[rowptr_t[j]:rowptr_t[j + 1]]
        same = col_t[rowptr_t[j]:rowptr_t[j + 1]]
        for a, b in zip(range(row.size - 1), range(1, row.size)):
            if same[a] == same[b]:
                assert row[b] == row[a] + 1


@pytest.mark.parametrize("case", cases.LAYER_CASES, ids=lambda c: c.id)
def test_layer_restatements_stay_within_the_rule_and_the_gate_share_under_the_cap(case):
    """The float32 restatements of out and every gradient sit near float32 rounding relative to the conditioning of the case, so
    FACTOR * err_32 is a threshold a legitimate kernel can meet; the edge form in float64 IS the dense reference; the reference alone
    keeps the gated share under the cap."""
    assert cases.gate_share(case) <= cases.EXCLUDED_CAP
    t64, err32, _, mismatches = cases.layer_expectation(case)
    assert mismatches is None
    assert set(err32) == {"out", "grad_x", "grad_lin_l.weight", "grad_att_l", "grad_att_r"} | ({"grad_bias"} if case.bias else set())
    bound = 2.0 ** -10 if case.att_scale != 1.0 else 2.0 ** -17
    for k, e in err32.items():
        assert 0 < e < bound, (k, e)
    conf = cases._conf(case)
    again = cases._layer_tensors(case, lambda x, w, al, ar, b: cases.edge_layer(case.graph, x, w, al, ar, b, *conf, 3), torch.float64)
    for k in t64:
        assert cases.err(again[k], t64[k]) < 1e-11, k
        assert bool(torch.isfinite(t64[k]).all())


def test_the_overflow_case_overflows_without_the_max_subtraction():
    e, terms, _ = cases.layer_gate(cases.OVERFLOW_CASE)
    top = e[terms].abs().max()
    with np.errstate(over="ignore"):
        assert float(top) > 150.0 and not np.isfinite(np.exp(np.float32(top)))


@pytest.mark.parametrize("case", (cases.LAYER_CASES[1], cases.LAYER_CASES[9]), ids=lambda c: c.id)
def test_rows_of_the_reference_alpha_sum_to_one_or_to_zero(case):
    g = cases.graph("main")
    alpha, alpha_self = cases.reference_alpha(case)
    rowptr, col = cases.canonical("main", False)
    rows = torch.from_numpy(np.repeat(np.arange(g.n), np.diff(rowptr)).astype(np.int64))
    total = torch.zeros((g.n, case.H), dtype=torch.float64).index_add_(0, rows, alpha) + alpha_self
    has_terms = torch.ones(g.n, dtype=torch.bool) if case.add_self_loops else torch.from_numpy(np.diff(rowptr) > 0)
    assert bool((~has_terms).any()) == (not case.add_self_loops)
    assert float((total[has_terms] - 1).abs().max()) < 1e-12 and float(total[~has_terms].abs().sum()) == 0.0
    if case.add_self_loops:
        loops = torch.from_numpy(col.astype(np.int64)) == rows
        assert int(loops.sum()) == 58 and float(alpha[loops].abs().sum()) == 0.0 and float(alpha_self.min()) > 0


def test_propagate_and_scores_restatements_against_float64():
    g = cases.graph("main")
    rowptr, col = cases.canonical("main", False)
    rs = np.random.RandomState(11)
    H, C = 3, 7
    h = (0.25 + rs.randn(g.n, H, C)).astype(np.float32)
    alpha = rs.rand(g.nnz, H).astype(np.float32)
    alpha_self = rs.rand(g.n, H).astype(np.float32)
    bias = rs.randn(H * C).astype(np.float32)
    rows = np.repeat(np.arange(g.n), np.diff(rowptr))
    for own in (alpha_self, None):
        a64 = alpha.astype(np.float64).copy()
        if own is not None:
            a64[col == rows] = 0.0
        want = np.zeros((g.n, H, C))
        np.add.at(want, rows, a64[:, :, None] * h[col].astype(np.float64))
        if own is not None:
            want += own[:, :, None].astype(np.float64) * h
        got = cases.propagate_restatement(rowptr, col, g.n, h, alpha, own, bias, True)
        assert cases.err(got, want.reshape(g.n, H * C) + bias) <= 16 * cases.FLOOR
        got = cases.propagate_restatement(rowptr, col, g.n, h, alpha, own, bias[:C], False)
        assert cases.err(got, want.sum(1) / H + bias[:C]) <= 16 * cases.FLOOR
    att = rs.randn(H, C).astype(np.float32)
    assert cases.err(cases.scores_restatement(h, att), (h.astype(np.float64) * att[None]).sum(-1)) <= 8 * cases.FLOOR


def test_model_reference_gate_and_restatements():
    ref, err32, share, mismatches = cases.model_expectation()
    assert mismatches is None and share <= cases.EXCLUDED_CAP
    assert set(err32) == {"logits"} | {"grad:" + k for k in cases.PARAMS}
    for k, e in err32.items():
        assert 0 < e < 2.0 ** -16, (k, e)
    assert np.isfinite(ref["loss"])


# ------------------------------------------------------------------------------------------------ host logic of the library

def test_argument_checks_of_every_entry_point(lib):
    from graphpope_amd import _lib
    f = p(FAKE)
    ok_fwd = dict(N=10, nnz=20, c_in=4, H=2, C=4, slope=0.2)

    def fwd(**kw):
        a = dict(ok_fwd, **kw)
        return lib.pope_gat_conv_forward(f, f, a["N"], a["nnz"], f, a["c_in"], f, f, f, None, a["H"], a["C"], 1, a["slope"], 1, f, f, f, f, f, f,
                                         kw.get("scratch", f), kw.get("bytes", 0), None)

    def bwd(**kw):
        a = dict(ok_fwd, **kw)
        return lib.pope_gat_conv_backward(f, f, f, f, f, a["N"], a["nnz"], f, a["c_in"], f, f, f, a["H"], a["C"], 1, a["slope"], 1, f, f, f, f, f,
                                          f, None, f, f, f, None, kw.get("scratch", f), kw.get("bytes", 0), None)

    bad = (dict(N=0), dict(N=2 ** 31 - 1), dict(nnz=-1), dict(nnz=2 ** 31 - 1), dict(c_in=0), dict(H=0), dict(C=0), dict(H=2 ** 15, C=2 ** 15),
           dict(slope=-0.1), dict(slope=1.5), dict(slope=float("nan")), dict(scratch=None))
    for kw in bad:
        assert fwd(**kw) == _lib.ERR_INVALID and b"pope_gat_conv_forward" in lib.pope_last_error(), kw
        assert bwd(**kw) == _lib.ERR_INVALID and b"pope_gat_conv_backward" in lib.pope_last_error(), kw
    # a short scratch: refused with the needed size, before anything is launched
    need = lib.pope_gat_conv_forward_scratch_size(10, 20, 4, 2, 4, 1)
    assert fwd(bytes=need - 1) == _lib.ERR_WORKSPACE and str(need).encode() in lib.pope_last_error()
    need = lib.pope_gat_conv_backward_scratch_size(10, 20, 4, 2, 4, 1)
    assert bwd(bytes=need - 1) == _lib.ERR_WORKSPACE and str(need).encode() in lib.pope_last_error()
    need = lib.pope_gat_propagate_scratch_size(10, 20, 2, 4, 0)
    assert lib.pope_gat_propagate(f, f, 10, 20, f, f, f, 2, 4, 0, None, p(8192), f, need - 1, None) == _lib.ERR_WORKSPACE
    assert lib.pope_gat_propagate(f, f, 10, 20, f, f, f, 2, 4, 1, None, f, f, 1 << 20, None) == _lib.ERR_INVALID and b"alias" in lib.pope_last_error()
    assert lib.pope_gat_propagate(f, f, 10, 20, None, f, f, 2, 4, 1, None, p(8192), f, 1 << 20, None) == _lib.ERR_INVALID
    assert lib.pope_gat_propagate(f, f, 0, 20, f, f, f, 2, 4, 1, None, p(8192), f, 1 << 20, None) == _lib.ERR_INVALID
    assert lib.pope_gat_attention(f, f, 10, 20, f, 2, 4, f, f, 0.2, 1, f, f, None, f, None) == _lib.ERR_INVALID
    assert lib.pope_gat_attention(f, f, 10, 20, f, 0, 4, f, f, 0.2, 1, f, f, f, f, None) == _lib.ERR_INVALID
    assert lib.pope_gat_attention(f, f, 10, 20, f, 2, 4, f, f, 2.0, 1, f, f, f, f, None) == _lib.ERR_INVALID and b"negative_slope" in lib.pope_last_error()
    assert lib.pope_gat_slot_map(f, f, None, f, 10, 20, f, None) == _lib.ERR_INVALID
    assert lib.pope_gat_slot_map(f, f, f, f, 0, 20, f, None) == _lib.ERR_INVALID and b"pope_gat_slot_map" in lib.pope_last_error()


def test_size_queries(lib):
    n, nnz = 89250, 899756
    for q in (lib.pope_gat_conv_forward_scratch_size, lib.pope_gat_conv_backward_scratch_size):
        assert q(0, nnz, 8, 8, 32, 1) == 0 and q(n, -1, 8, 8, 32, 1) == 0 and q(n, nnz, 0, 8, 32, 1) == 0 and q(n, nnz, 8, 0, 32, 1) == 0
        assert q(n, nnz, 8, 8, 0, 1) == 0 and q(n, nnz, 8, 2 ** 15, 2 ** 15, 1) == 0 and q(2 ** 31 - 1, nnz, 8, 8, 32, 1) == 0
        assert q(n, nnz, 8, 8, 32, 1) % 256 == 0
    assert lib.pope_gat_propagate_scratch_size(0, nnz, 8, 32, 1) == 0 and lib.pope_gat_propagate_scratch_size(n, nnz, 0, 32, 1) == 0
    cat, mean = (lib.pope_gat_propagate_scratch_size(n, nnz, 8, 32, c) for c in (1, 0))
    assert mean - cat == n * 256 * 4 and cat > 0                     # the head mean reads the concatenated rows from scratch
    assert lib.pope_gat_conv_forward_scratch_size(n, nnz, 500, 8, 32, 1) == cat
    back = lib.pope_gat_conv_backward_scratch_size(n, nnz, 500, 8, 32, 1)
    assert back >= nnz * 8 * 4 + n * 256 * 4 + 3 * n * 8 * 4
    assert lib.pope_gat_conv_backward_scratch_size(n, nnz, 500, 8, 32, 0) - back == n * 256 * 4
    # no row can be a hub: the counters alone
    assert lib.pope_gat_propagate_scratch_size(17, 0, 2, 4, 1) == 256


def test_kernel_names_follow_the_shapes(lib):
    buf = ctypes.create_string_buffer(768)

    def name(n, nnz, c_in, H, C, concat=1, backward=0, grad_x=1, mis=0, cap=768):
        from graphpope_amd import _lib
        _lib.check(lib.pope_gat_kernel_name(n, nnz, c_in, H, C, concat, backward, grad_x, cases.CUS, mis, buf, cap))
        return buf.value.decode().split("+")

    g = cases.graph("main")
    fwd = name(g.n, g.nnz, 36, 4, 64)
    assert fwd[0].startswith("k_gemm<") and fwd[1:] == ["k_gat_scores", "k_gat_attention", "k_gcn_clear", "k_gat_propagate<true, false>",
                                                        "k_gat_hub_partial<true, false>", "k_gat_hub_finish<true, false>"]
    assert name(g.n, g.nnz, 36, 4, 64, concat=0)[-1] == "k_gat_head_mean"
    assert "k_gat_propagate<false, true>" in name(g.n, g.nnz, 36, 8, 8) and "k_gat_propagate<false, true>" in name(g.n, g.nnz, 37, 1, 5)
    assert "k_gat_propagate<false, false>" in name(g.n, g.nnz, 36, 1, 130)                  # a width that is no multiple of 4
    assert "k_gat_propagate<true, false>" in name(g.n, g.nnz, 36, 2, 130)
    for bit in (2, 3, 5):                                                                   # h, out, scratch off the 16-byte grid
        assert "k_gat_propagate<false, false>" in name(g.n, g.nnz, 36, 4, 64, mis=1 << bit)
    assert "k_gat_propagate<true, false>" in name(g.n, g.nnz, 36, 4, 64, mis=0b10011)       # x, weight, grad_x: not the propagate's
    assert "k_gcn_clear" not in name(17, 0, 36, 4, 64) and "k_gcn_clear" not in name(g.n, cases.CHUNK, 36, 4, 64)
    assert name(89250, 899756, 500, 8, 32)[0].startswith("k_gemm_tile16<")
    bwd = name(g.n, g.nnz, 36, 4, 64, backward=1)
    assert bwd[:2] == ["k_gat_edge_grad", "k_gat_src_grad"] and bwd[2:6] == ["k_gcn_clear", "k_gat_propagate<true, false>",
                                                                            "k_gat_hub_partial<true, false>", "k_gat_hub_finish<true, false>"]
    assert bwd[6:9] == ["k_gat_att_partial", "k_colsum_final", "k_colsum_final"] and "[splits=" in bwd[9] and bwd[10] == "k_slab_reduce"
    assert bwd[11].startswith("k_gemm<") and bwd[12:] == ["k_colsum_partial<true>", "k_colsum_final"]
    nogx = name(g.n, g.nnz, 36, 4, 64, backward=1, grad_x=0)
    assert len(nogx) == len(bwd) - 1
    assert name(g.n, g.nnz, 36, 4, 64, concat=0, backward=1)[0] == "k_gat_spread_grad"
    assert lib.pope_gat_kernel_name(0, 5, 4, 1, 4, 1, 0, 1, 256, 0, buf, 768) != 0
    assert lib.pope_gat_kernel_name(5, 5, 4, 1, 4, 1, 0, 1, 256, 1 << 6, buf, 768) != 0
    assert lib.pope_gat_kernel_name(5, 5, 4, 1, 4, 1, 0, 1, 0, 0, buf, 768) != 0
    assert lib.pope_gat_kernel_name(g.n, g.nnz, 36, 4, 64, 1, 1, 1, 256, 0, buf, 16) != 0 and b"do not fit" in lib.pope_last_error()


# ------------------------------------------------------------------------------------------------ the Python layer

def test_constructor_parameters_and_repr():
    from graphpope_amd import gat
    conv = gat.GATConv(12, 7, heads=3)
    assert [k for k, _ in conv.named_parameters()] == ["att_l", "att_r", "bias", "lin_l.weight"]
    assert sorted(conv.state_dict()) == ["att_l", "att_r", "bias", "lin_l.weight"]
    assert conv.lin_l.weight.shape == (21, 12) and conv.att_l.shape == conv.att_r.shape == (1, 3, 7) and conv.bias.shape == (21,)
    assert conv.lin_r is conv.lin_l and conv.lin_l.bias is None
    assert float(conv.bias.detach().abs().sum()) == 0.0 and float(conv.lin_l.weight.detach().abs().max()) <= np.sqrt(6.0 / (12 + 21))
    assert 0 < float(conv.att_l.detach().abs().max()) <= np.sqrt(6.0 / (3 + 7))
    assert conv.extra_repr() == "12, 7, heads=3" and repr(conv).startswith("GATConv(")
    assert (conv.concat, conv.negative_slope, conv.dropout, conv.add_self_loops) == (True, 0.2, 0.0, True)
    mean = gat.GATConv(12, 7, heads=3, concat=False, bias=False)
    assert mean.bias is None and gat.GATConv(12, 7, heads=3, concat=False).bias.shape == (7,)
    with pytest.raises(ValueError):
        gat.GATConv(12, 7, heads=0)
    with pytest.raises(ValueError, match="negative_slope"):
        gat.GATConv(12, 7, negative_slope=1.5)


def test_gat_model_layers_and_hidden_not_a_multiple_of_heads():
    from graphpope_amd import gat
    model = gat.GAT(36, 64, 5, num_layers=3, heads=8, dropout=0.5)
    assert [(c.in_channels, c.out_channels, c.heads) for c in model.convs] == [(36, 8, 8), (64, 8, 8), (64, 5, 1)]
    assert all(c.dropout == 0.0 and c.concat for c in model.convs) and model.dropout == 0.5
    assert len(gat.GAT(36, 64, 5, num_layers=1).convs) == 1
    with pytest.raises(ValueError, match="heads"):
        gat.GAT(36, 60, 5, heads=8)
    with pytest.raises(ValueError, match="num_layers"):
        gat.GAT(36, 64, 5, num_layers=0)


def test_attention_dropout_in_training_mode_is_refused_by_name():
    from graphpope_amd import gat
    conv = gat.GATConv(4, 4, dropout=0.3)
    assert conv.dropout == 0.3
    conv.train()
    with pytest.raises(NotImplementedError, match="dropout"):
        conv(torch.zeros(3, 4), None)
    conv.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # past the refusal: the layer itself runs on the GPU only
        conv(torch.zeros(3, 4), None)


def test_layer_and_heads_switches_are_checked_before_the_gpu_is_touched(monkeypatch):
    from graphpope_amd import main
    assert main.gcn_layer_from_env(256, {}) == ("gcn", 0)
    assert main.gcn_layer_from_env(256, {"GRAPHPOPE_GCN_LAYER": "gcn", "GRAPHPOPE_GAT_HEADS": "7"}) == ("gcn", 0)
    assert main.gcn_layer_from_env(256, {"GRAPHPOPE_GCN_LAYER": "gat"}) == ("gat", 8)
    assert main.gcn_layer_from_env(60, {"GRAPHPOPE_GCN_LAYER": "gat", "GRAPHPOPE_GAT_HEADS": "4"}) == ("gat", 4)
    with pytest.raises(ValueError, match="GRAPHPOPE_GCN_LAYER"):
        main.gcn_layer_from_env(256, {"GRAPHPOPE_GCN_LAYER": "sage"})
    for heads in ("7", "0", "-2", "many"):
        with pytest.raises(ValueError, match="GRAPHPOPE_GAT_HEADS"):
            main.gcn_layer_from_env(256, {"GRAPHPOPE_GCN_LAYER": "gat", "GRAPHPOPE_GAT_HEADS": heads})
    # the command line refuses both before any device work (torch.cuda is never asked: there is no GPU here or it is not needed)
    monkeypatch.setenv("GRAPHPOPE_MODEL", "gcn")
    monkeypatch.setenv("GRAPHPOPE_GCN_LAYER", "transformer")
    with pytest.raises(ValueError, match="GRAPHPOPE_GCN_LAYER"):
        main.main(["--dataset", "pubmed", "--epochs", "1"])
    monkeypatch.setenv("GRAPHPOPE_GCN_LAYER", "gat")
    monkeypatch.setenv("GRAPHPOPE_GAT_HEADS", "7")
    with pytest.raises(ValueError, match="GRAPHPOPE_GAT_HEADS"):
        main.main(["--dataset", "pubmed", "--epochs", "1", "--hidden_layer_size", "256"])
    monkeypatch.setenv("GRAPHPOPE_MODEL", "gat")
    with pytest.raises(ValueError, match="expected sage or gcn"):
        main.model_from_env()
