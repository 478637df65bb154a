"""GCNConv / GCN without a GPU, through tests/gcn_cases.py: the restatements against the float64 reference within the rule, the graph's
asymmetry, and everything of pope_gcn_* and graphpope_amd/gcn.py that is host logic -- argument checks of all eight entry points, the
size and name queries, the constructor, the GRAPHPOPE_MODEL switch."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import gcn_cases as cases


@pytest.fixture(scope="module")
def lib():
    from graphpope_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _leave_no_error_string_behind(lib):
    """The refusals tested here set pope_last_error; a successful query clears it, so that no later test of the process finds it."""
    yield
    buf = ctypes.create_string_buffer(512)
    assert lib.pope_gcn_kernel_name(1, 0, 4, 4, 0, 1, 256, 0, buf, 512) == 0 and lib.pope_last_error() == b""


def p(v):
    return ctypes.c_void_p(v)


FAKE = 4096                       # a pointer that is never dereferenced: validation happens before anything touches the device


# ------------------------------------------------------------------------------------------------ the reference side

def test_the_graph_is_the_documented_one_and_asymmetric():
    g = cases.graph("main")
    assert (g.n, g.nnz) == (300, 4029) and int((g.col == g.dst).sum()) == 58
    deg = np.diff(g.rowptr)
    assert set(cases.fic.DEGREES) <= set(deg.tolist()) and deg.max() == 2 * cases.CHUNK + 1
    rowptr_t, col_t = cases.transposed("main")
    assert rowptr_t[-1] == g.nnz and col_t.size == g.nnz
    # by source and by destination differ: a backward pass over the wrong one cannot pass unnoticed
    assert not np.array_equal(rowptr_t, g.rowptr)
    assert not np.array_equal(np.diff(rowptr_t), deg)
    for i in range(g.n):                                             # canonical rows: ascending
        assert (np.diff(col_t[rowptr_t[i]:rowptr_t[i + 1]]) >= 0).all()
    # the transpose holds the same multiset of edges
    src_t = np.repeat(np.arange(g.n), np.diff(rowptr_t))
    assert sorted(zip(src_t.tolist(), col_t.tolist())) == sorted(zip(g.src.tolist(), g.dst.tolist()))
    # the run structure the contract speaks of: a hub row whose self-loop slot is skipped but keeps its position
    hub = g.special[cases.CHUNK + 1]
    assert g.col[g.rowptr[hub]] == hub


@pytest.mark.parametrize("improved,add_self_loops", cases.SETTINGS)
def test_dinv_restatement_is_the_dense_normalisation(improved, add_self_loops):
    g, f = cases.graph("main"), cases.self_weight(improved, add_self_loops)
    dinv = cases.dinv_restatement(g.rowptr, g.col, g.n, f)
    a = torch.zeros((g.n, g.n), dtype=torch.float64)
    a.index_put_((torch.from_numpy(g.dst), torch.from_numpy(g.src)), torch.ones(g.nnz, dtype=torch.float64), accumulate=True)
    if f > 0:
        a.fill_diagonal_(f)
    deg = a.sum(1).numpy()
    want = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1e-300)), 0.0)
    assert np.abs(dinv - want).max() <= 2.0 ** -24 * want.max()
    assert (dinv == 0).sum() == (deg == 0).sum() and ((deg == 0).sum() > 0) == (f == 0)


@pytest.mark.parametrize("by_source", (False, True))
@pytest.mark.parametrize("improved,add_self_loops", cases.SETTINGS[:3])
def test_propagate_restatement_against_the_dense_product(by_source, improved, add_self_loops):
    """The documented order, in float32, is the dense float64 product within the rule's floor times the row length."""
    g, f = cases.graph("main"), cases.self_weight(improved, add_self_loops)
    rowptr, col = cases.csr("main", by_source)
    dinv = cases.dinv_restatement(g.rowptr, g.col, g.n, f)          # the SAME vector for both directions
    h = (0.25 + np.random.RandomState(3).randn(g.n, 7)).astype(np.float32)
    b = np.random.RandomState(4).randn(7).astype(np.float32)
    got = cases.propagate_restatement(rowptr, col, g.n, h, dinv, f, b)
    a_hat = cases.dense_adjacency("main", True, f)
    want = (a_hat.T if by_source else a_hat) @ torch.from_numpy(h).double() + torch.from_numpy(b).double()
    assert cases.err(got, want) <= 16 * cases.FLOOR
    plain = cases.propagate_restatement(rowptr, col, g.n, h)
    a = cases.dense_adjacency("main", False, 0.0)
    assert cases.err(plain, (a.T if by_source else a) @ torch.from_numpy(h).double()) <= 16 * cases.FLOOR


def test_empty_graph_with_unit_self_weight_returns_h_plus_b():
    g = cases.graph("empty")
    h = np.random.RandomState(5).randn(g.n, 7).astype(np.float32)
    b = np.random.RandomState(6).randn(7).astype(np.float32)
    dinv = cases.dinv_restatement(g.rowptr, g.col, g.n, 1.0)
    assert (dinv == 1).all()
    assert np.array_equal(cases.propagate_restatement(g.rowptr, g.col, g.n, h, dinv, 1.0, b), h + b)


@pytest.mark.parametrize("case", cases.LAYER_CASES, ids=lambda c: c.id)
def test_layer_restatements_stay_within_the_rule(case):
    """The float32 restatements of out and every gradient sit near float32 rounding, so FACTOR * err_32 is a threshold a legitimate
    kernel can meet and a wrong one cannot: every err_32 is below 2^-18, and the edge form in float64 IS the dense reference."""
    t64, err32 = cases.layer_expectation(case)
    assert set(err32) == {"out", "grad_x", "grad_weight"} | ({"grad_bias"} if case.bias else set())
    for k, e in err32.items():
        assert 0 < e < 2.0 ** -18, (k, e)
    again = cases._layer_tensors(case, lambda x, w, b: cases.edge_layer(case.graph, x, w, b, case.normalize, case.f, "project", 3), torch.float64)
    for k in t64:
        assert cases.err(again[k], t64[k]) < 1e-13, k


def test_model_reference_gate_and_restatements():
    z, gated = cases.model_gate()
    assert int(gated.sum()) <= cases.EXCLUDED_CAP * z.numel()       # the float64 reference alone stays inside the cap
    ref, err32, n_gated, mismatches = cases.model_expectation()
    assert mismatches is None and n_gated == int(gated.sum())
    assert set(err32) == {"logits"} | {"grad:" + k for k in cases.PARAMS}
    for k, e in err32.items():
        assert 0 < e < 2.0 ** -17, (k, e)
    # a flipped pattern element outside the gate moves the gradients by far more than the threshold
    far = (~gated & (z > 0)).nonzero()[0]
    pattern = (z > 0).clone()
    pattern[far[0], far[1]] = False
    moved = cases.model_run(torch.float64, pattern)
    assert cases.err(moved["grad:convs.0.weight"], ref["grad:convs.0.weight"]) > cases.threshold(err32["grad:convs.0.weight"])
    assert cases.loss_bound(ref, err32) < 1e-4


# ------------------------------------------------------------------------------------------------ host logic of the library

def _propagate(lib, **over):
    a = dict(rowptr=FAKE, col=FAKE, N=10, nnz=20, dinv=FAKE, f=1.0, h=FAKE, C=8, bias=FAKE, out=8192, scratch=FAKE, bytes=1 << 30)
    a.update(over)
    return lib.pope_gcn_propagate(p(a["rowptr"]), p(a["col"]), a["N"], a["nnz"], p(a["dinv"]), a["f"], p(a["h"]), a["C"], p(a["bias"]), p(a["out"]),
                                  p(a["scratch"]), a["bytes"], None)


def _forward(lib, **over):
    a = dict(rowptr=FAKE, col=FAKE, N=10, nnz=20, dinv=FAKE, f=1.0, x=FAKE, c_in=8, weight=FAKE, bias=FAKE, c_out=8, out=FAKE, scratch=FAKE,
             bytes=1 << 30)
    a.update(over)
    return lib.pope_gcn_conv_forward(p(a["rowptr"]), p(a["col"]), a["N"], a["nnz"], p(a["dinv"]), a["f"], p(a["x"]), a["c_in"], p(a["weight"]),
                                     p(a["bias"]), a["c_out"], p(a["out"]), p(a["scratch"]), a["bytes"], None)


def _backward(lib, **over):
    a = dict(rowptr=FAKE, col=FAKE, N=10, nnz=20, dinv=FAKE, f=1.0, x=FAKE, c_in=8, weight=FAKE, c_out=8, grad_out=FAKE, grad_x=FAKE,
             grad_weight=FAKE, grad_bias=FAKE, scratch=FAKE, bytes=1 << 30)
    a.update(over)
    return lib.pope_gcn_conv_backward(p(a["rowptr"]), p(a["col"]), a["N"], a["nnz"], p(a["dinv"]), a["f"], p(a["x"]), a["c_in"], p(a["weight"]),
                                      a["c_out"], p(a["grad_out"]), p(a["grad_x"]), p(a["grad_weight"]), p(a["grad_bias"]), p(a["scratch"]),
                                      a["bytes"], None)


def test_argument_checks_need_no_gpu(lib):
    from graphpope_amd import _lib
    bad_sizes = (dict(N=0), dict(N=-1), dict(N=2 ** 31 - 1), dict(nnz=-1), dict(nnz=2 ** 31 - 1), dict(f=-1.0), dict(f=float("nan")))
    calls = ((_propagate, "pope_gcn_propagate", ("rowptr", "col", "h", "out", "scratch"), (dict(C=0),)),
             (_forward, "pope_gcn_conv_forward", ("rowptr", "col", "x", "weight", "out", "scratch"), (dict(c_in=0), dict(c_out=-3))),
             (_backward, "pope_gcn_conv_backward", ("rowptr", "col", "x", "weight", "grad_out", "grad_weight", "scratch"), (dict(c_in=0), dict(c_out=0))))
    for call, name, pointers, widths in calls:
        for key in pointers:
            assert call(lib, **{key: 0}) == _lib.ERR_INVALID, (name, key)
            assert name.encode() in lib.pope_last_error() and b"null pointer" in lib.pope_last_error()
        for over in bad_sizes + widths:
            assert call(lib, **over) == _lib.ERR_INVALID, (name, over)
            assert name.encode() in lib.pope_last_error()
    assert _propagate(lib, out=FAKE) == _lib.ERR_INVALID and b"alias" in lib.pope_last_error()
    # the degree pass
    deg = lambda **o: lib.pope_gcn_degree_norm(p(o.get("rowptr", FAKE)), p(o.get("col", FAKE)), o.get("N", 10), o.get("nnz", 20), o.get("f", 1.0),  # noqa: E731
                                               p(o.get("dinv", FAKE)), None)
    for over in (dict(rowptr=0), dict(col=0), dict(dinv=0), dict(N=0), dict(nnz=-1), dict(f=-0.5), dict(f=float("inf"))):
        assert deg(**over) == _lib.ERR_INVALID, over
        assert b"pope_gcn_degree_norm" in lib.pope_last_error()
    # one byte short: POPE_ERR_WORKSPACE with both sizes in the message, before any HIP call (none could succeed here)
    for call, query, args in ((_propagate, lib.pope_gcn_propagate_scratch_size, (10, 20, 8)),
                              (_forward, lib.pope_gcn_conv_forward_scratch_size, (10, 20, 8, 8)),
                              (_backward, lib.pope_gcn_conv_backward_scratch_size, (10, 20, 8, 8))):
        need = query(*args)
        assert need > 0 and call(lib, bytes=need - 1) == _lib.ERR_WORKSPACE
        assert str(need).encode() in lib.pope_last_error() and str(need - 1).encode() in lib.pope_last_error()


def test_scratch_queries_are_monotone_and_zero_for_refused_shapes(lib):
    big = 2 ** 31 - 2
    queries = ((lib.pope_gcn_propagate_scratch_size, (201, 400, 5), [(0, 4, 4), (-1, 4, 4), (5, -1, 4), (5, 4, 0), (2 ** 31 - 1, 4, 4), (5, 2 ** 31 - 1, 4)]),
               (lib.pope_gcn_conv_forward_scratch_size, (201, 400, 5, 6), [(0, 4, 4, 4), (5, -1, 4, 4), (5, 4, 0, 4), (5, 4, 4, 0), (2 ** 31 - 1, 4, 4, 4)]),
               (lib.pope_gcn_conv_backward_scratch_size, (201, 400, 5, 6), [(0, 4, 4, 4), (5, -1, 4, 4), (5, 4, 0, 4), (5, 4, 4, 0), (2 ** 31 - 1, 4, 4, 4)]))
    for q, base, rejected in queries:
        assert q(*base) > 0
        for args in rejected:
            assert q(*args) == 0, args
        for i in range(len(base)):
            args, prev, steps = list(base), q(*base), 0
            while args[i] * 2 <= big:
                args[i] *= 2
                now = q(*args)
                assert now >= prev > 0, (tuple(args), prev, now)
                prev, steps = now, steps + 1
            assert steps >= 15 and prev < 2 ** 62
    # the layout is a function of the sizes alone: the hub region appears with the first row that could be a hub
    q = lib.pope_gcn_propagate_scratch_size
    assert q(300, cases.CHUNK, 64) == 256 and q(300, cases.CHUNK + 1, 64) > 256


def _name(lib, n, nnz, c_in, c_out, backward=0, grad_x=1, mask=0, cap=512):
    from graphpope_amd import _lib
    buf = ctypes.create_string_buffer(cap)
    _lib.check(lib.pope_gcn_kernel_name(n, nnz, c_in, c_out, backward, grad_x, cases.CUS, mask, buf, cap))
    return buf.value.decode()


# the propagate's three forms <VEC, NARROW>: 16-byte accesses, four scalar columns per lane, and for c_out <= 64 one column per lane
HUBS = "k_gcn_clear+k_gcn_propagate<%s>+k_gcn_hub_partial<%s>+k_gcn_hub_finish<%s>"
HUBS_V, HUBS_S, HUBS_N = (HUBS % (f, f, f) for f in ("true, false", "false, false", "false, true"))
# (c_in, c_out) -> the forward launches on the test graph.  The whole-tile projection needs full_plan's conditions: depth % 4 == 0, at
# least 64 Ki outputs, and t16_pick_rb's 30 % utilisation of one round of 16-row tiles, which 300 rows reach from c_out = 525 on -- so
# the five shapes of the layer tests take the plain tile kernel (reading W where it lies: layouts 1, 2 = depth-contiguous x, outer-
# contiguous W; 0, 0 where a width is no multiple of 4) and WHOLE_TILE_SHAPE is there to reach the other path.
FORWARD_NAMES = {
    (36, 256): "k_gemm<64, 64, 2, 2, 1, 2>+" + HUBS_V,
    (36, 260): "k_gemm<64, 64, 2, 2, 1, 2>+" + HUBS_V,
    (12, 7): "k_gemm<64, 64, 2, 2, 0, 0>+" + HUBS_N,
    (256, 512): "k_gemm<64, 64, 2, 2, 1, 2>+" + HUBS_V,
    (37, 64): "k_gemm<64, 64, 2, 2, 0, 0>+" + HUBS_N,
    cases.WHOLE_TILE_SHAPE: "k_gcn_transpose+k_gemm_tile16<1, 4>+" + HUBS_V,
}


def test_kernel_name_query_prints_the_plan(lib):
    from graphpope_amd import _lib
    g = cases.graph("main")
    for (c_in, c_out), want in FORWARD_NAMES.items():
        assert _name(lib, g.n, g.nnz, c_in, c_out) == want, (c_in, c_out)
    # a graph without a possible hub has no hub launches; misaligned out or scratch takes the scalar propagate, misaligned x the plain tiles
    assert set(FORWARD_NAMES) == set(cases.SHAPES) | {cases.WHOLE_TILE_SHAPE}
    assert _name(lib, 300, cases.CHUNK, 36, 640) == "k_gcn_transpose+k_gemm_tile16<1, 4>+k_gcn_propagate<true, false>"
    assert _name(lib, 300, cases.CHUNK, 36, 640, mask=1 << 2) == "k_gcn_transpose+k_gemm_tile16<1, 4>+k_gcn_propagate<false, false>"
    assert _name(lib, 300, cases.CHUNK, 36, 640, mask=1) == "k_gemm<64, 64, 2, 2, 0, 0>+k_gcn_propagate<true, false>"        # x off the grid
    assert _name(lib, 300, cases.CHUNK, 36, 640, mask=1 << 4) == "k_gemm<64, 64, 2, 2, 1, 2>+k_gcn_propagate<false, false>"   # the scratch
    assert _name(lib, 300, cases.CHUNK, 36, 64) == "k_gemm<64, 64, 2, 2, 1, 2>+k_gcn_propagate<false, true>"
    assert _name(lib, 300, cases.CHUNK, 36, 64, mask=1 << 2) == "k_gemm<64, 64, 2, 2, 1, 2>+k_gcn_propagate<false, true>"     # narrow whatever the alignment
    assert _name(lib, 300, cases.CHUNK, 36, 68) == "k_gemm<64, 64, 2, 2, 1, 2>+k_gcn_propagate<true, false>"                  # 65 columns on: four per lane
    # backward: propagate, split weight gradient, grad_x only when asked for, the two column-sum launches
    b = _name(lib, g.n, g.nnz, 36, 256, backward=1)
    assert b == HUBS_V + "+k_gemm<64, 64, 2, 2, 2, 2>[splits=2]+k_slab_reduce+k_gemm<64, 64, 2, 2, 1, 1>+k_colsum_partial<true>+k_colsum_final"
    assert _name(lib, g.n, g.nnz, 36, 256, backward=1, grad_x=0) == b.replace("+k_gemm<64, 64, 2, 2, 1, 1>", "")
    assert _name(lib, g.n, g.nnz, 12, 7, backward=1) == HUBS_N + ("+k_gemm<64, 64, 2, 2, 0, 0>[splits=2]+k_slab_reduce+k_gemm<64, 64, 2, 2, 0, 0>"
                                                                  "+k_colsum_partial<false>+k_colsum_final")
    flickr = _name(lib, 89250, 899756, 756, 256)
    assert flickr.startswith("k_gcn_transpose+k_gemm_tile16<") and flickr.endswith(HUBS_V)
    buf = ctypes.create_string_buffer(512)
    for bad in ((0, 4, 4, 4, 0, 1, 256, 0), (5, -1, 4, 4, 0, 1, 256, 0), (5, 4, 0, 4, 0, 1, 256, 0), (5, 4, 4, 0, 0, 1, 256, 0), (5, 4, 4, 4, 0, 1, 0, 0),
                (5, 4, 4, 4, 0, 1, 256, 1 << 5)):
        assert lib.pope_gcn_kernel_name(*bad, buf, 512) == _lib.ERR_INVALID, bad
    assert lib.pope_gcn_kernel_name(300, 10, 36, 256, 0, 1, 256, 0, None, 512) == _lib.ERR_INVALID
    assert lib.pope_gcn_kernel_name(300, 10, 36, 256, 0, 1, 256, 0, buf, 8) == _lib.ERR_INVALID and b"do not fit" in lib.pope_last_error()


def test_the_contract_is_in_the_header_and_the_kernels_in_gcn_h():
    from conftest import ROOT
    import os
    header = open(os.path.join(ROOT, "include", "graphpope_hip.h")).read()
    assert "The summation contract" in header and "CHUNK = %d" % cases.CHUNK in header
    source = open(os.path.join(ROOT, "graphpope_amd", "csrc", "gcn.h")).read()
    for kernel in ("k_gcn_degree_norm", "k_gcn_propagate", "k_gcn_hub_partial", "k_gcn_hub_finish"):
        assert "void " + kernel + "(" in source
    assert all("counters" in line for line in source.splitlines() if "atomicAdd(" in line)       # integer list counters, no float atomics
    assert '#include "gcn.h"' in open(os.path.join(ROOT, "graphpope_amd", "csrc", "sage.hip")).read()


# ------------------------------------------------------------------------------------------------ the Python layer

def test_constructor_signature_state_dict_and_init():
    from graphpope_amd import gcn
    sig = inspect.signature(gcn.GCNConv.__init__)
    assert [(n, q.default) for n, q in list(sig.parameters.items())[1:]] == [
        ("in_channels", inspect.Parameter.empty), ("out_channels", inspect.Parameter.empty), ("improved", False), ("cached", False),
        ("add_self_loops", True), ("normalize", True), ("bias", True)]
    torch.manual_seed(0)
    conv = gcn.GCNConv(36, 64)
    state = conv.state_dict()
    assert list(state) == ["weight", "bias"] and state["weight"].shape == (36, 64) and state["bias"].shape == (64,)
    bound = (6.0 / (36 + 64)) ** 0.5                                 # glorot-uniform
    w = state["weight"]
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.95 * bound and abs(float(w.mean())) < 0.05 * bound
    assert abs(float(w.std()) - bound / 3 ** 0.5) < 0.1 * bound and bool((state["bias"] == 0).all())
    assert list(gcn.GCNConv(5, 3, bias=False, cached=True).state_dict()) == ["weight"]
    model = gcn.GCN(36, 64, 5, num_layers=3, dropout=0.25, improved=True)
    assert list(model.state_dict()) == [f"convs.{i}.{k}" for i in range(3) for k in ("weight", "bias")]
    assert [tuple(c.weight.shape) for c in model.convs] == [(36, 64), (64, 64), (64, 5)] and all(c.improved for c in model.convs)
    assert inspect.signature(gcn.GCN.__init__).parameters["num_layers"].default == 2
    assert inspect.signature(gcn.GCN.__init__).parameters["dropout"].default == 0.5
    with pytest.raises(ValueError):
        gcn.GCN(4, 4, 4, num_layers=0)


def test_gcnconv_refuses_the_cpu():
    from graphpope_amd import gcn
    conv = gcn.GCNConv(4, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        conv(torch.zeros(5, 4), None)


def test_model_switch_is_checked_before_the_gpu_is_touched(monkeypatch):
    from graphpope_amd import main
    assert main.model_from_env({}) == "sage" and main.model_from_env({"GRAPHPOPE_MODEL": "gcn"}) == "gcn"
    with pytest.raises(ValueError, match="GRAPHPOPE_MODEL"):
        main.model_from_env({"GRAPHPOPE_MODEL": "gat"})
    monkeypatch.setattr(main, "_main", lambda *a, **k: pytest.fail("the run started"))
    monkeypatch.setattr(main, "_launch_ranks", lambda *a, **k: pytest.fail("ranks were started"))
    monkeypatch.setenv("GRAPHPOPE_MODEL", "gat")
    with pytest.raises(ValueError, match="expected sage or gcn"):
        main.main(["--epochs", "1"])
    monkeypatch.setenv("GRAPHPOPE_MODEL", "gcn")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match="n_gpus"):
        main.main(["--epochs", "1", "--n_gpus", "2"])
