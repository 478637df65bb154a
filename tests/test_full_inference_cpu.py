"""Exact full-graph SAGE inference without a GPU: the reference of tests/full_inference_cases.py against a dense formulation, the case
graph, the threshold, and everything of sage_full_layer_* and SAGE.inference that is host logic (size and name queries, argument
validation, the GPU-only error, the flag surface of the command line)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import full_inference_cases as cases

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from graphpope_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _leave_no_error_message_behind(lib):
    """The refusals provoked here set pope_last_error; a call that succeeds clears it again for whichever test runs next."""
    yield
    buf = ctypes.create_string_buffer(384)
    assert lib.sage_full_layer_kernel_name(1, 0, 4, 4, 0, cases.CUS, 0, buf, 384) == 0 and lib.pope_last_error() == b""


def _dense_mean(g):
    a = np.zeros((g.n, g.n), dtype=np.float64)
    np.add.at(a, (g.dst, g.src), 1.0)                               # repeated edges count as often as they occur
    return torch.from_numpy(a / np.maximum(a.sum(1, keepdims=True), 1.0))


def _dense_layer(g, h, w_l, b_l, w_r, bn):
    out = _dense_mean(g) @ h @ w_l.T + b_l + h @ w_r.T
    if bn is not None:
        gamma, beta, mean, var = bn
        out = torch.clamp((out - mean) * (var + cases.EPS) ** -0.5 * gamma + beta, min=0)
    return out


@pytest.mark.parametrize("case", cases.LAYER_CASES, ids=lambda c: c.id)
def test_layer_reference_equals_the_dense_formulation(case):
    g = cases.graph(case.graph)
    t = {k: torch.from_numpy(v).double() for k, v in cases.layer_inputs(case).items()}
    bn = (t["gamma"], t["beta"], t["mean"], t["var"]) if case.has_bn else None
    want = _dense_layer(g, t["x"], t["w_l"], t["b_l"], t["w_r"], bn)
    got = cases.layer_reference(case)
    assert got.dtype == torch.float64 and got.shape == (g.n, case.c_out)
    assert cases.err(got, want) <= 1e-12
    assert cases.err(cases.layer_reference(case, order="project", perm_seed=2), want) <= 1e-12


@pytest.mark.parametrize("num_layers, hops", cases.MODELS)
def test_model_reference_equals_the_dense_formulation(num_layers, hops):
    g, state = cases.graph("main"), cases.model_state(num_layers)
    h = torch.from_numpy(cases.model_x()).double()
    for i in range(hops):
        bn = tuple(state[f"bns.{i}.{k}"].double() for k in ("weight", "bias", "running_mean", "running_var")) if i < hops - 1 else None
        h = _dense_layer(g, h, state[f"convs.{i}.lin_l.weight"].double(), state[f"convs.{i}.lin_l.bias"].double(),
                         state[f"convs.{i}.lin_r.weight"].double(), bn)
    got = cases.model_reference(num_layers, hops)
    assert got.shape == (cases.N, cases.MODEL_OUT if hops == num_layers else cases.MODEL_HIDDEN)     # the depth quirk: hidden-wide logits
    assert cases.err(got, h) <= 1e-12


def test_case_graph_has_the_listed_degrees():
    g = cases.graph("main")
    deg = np.diff(g.rowptr)
    assert g.n == cases.N == 300 and g.n < cases.CHUNK and g.rowptr[0] == 0 and g.rowptr[-1] == g.nnz
    assert cases.DEGREES == (0, 1, 3, 4, 5, 8, 9, 64, 65, cases.CHUNK, cases.CHUNK + 1, 2 * cases.CHUNK + 1)
    for d in cases.DEGREES:
        assert deg[g.special[d]] == d
    assert g.col.min() >= 0 and g.col.max() < g.n
    assert (g.src == g.dst).sum() >= 10                             # self-loops
    hub = g.special[2 * cases.CHUNK + 1]
    assert np.unique(g.col[g.rowptr[hub]:g.rowptr[hub + 1]]).size < 2 * cases.CHUNK + 1       # a multigraph: duplicates supply the long rows
    assert (deg > cases.CHUNK).sum() == 2 and np.median(deg) <= 12
    assert sorted(np.flatnonzero(deg > 12)) == sorted(g.special[d] for d in cases.DEGREES if d > 12)   # spread over the ids, nothing else long
    for name, n in (("single", 1), ("empty", 17)):
        e = cases.graph(name)
        assert e.n == n and e.nnz == 0 and not e.rowptr.any()


@pytest.mark.parametrize("case", [c for c in cases.LAYER_CASES if c.graph == "main"], ids=lambda c: c.id)
def test_layer_restatement_error_is_neither_zero_nor_large(case):
    _, e32 = cases.layer_expectation(case)
    assert 0 < e32 < 1e-4, e32
    assert cases.layer_threshold(case) == cases.FACTOR * max(e32, 2.0 ** -23)


@pytest.mark.parametrize("num_layers, hops", cases.MODELS)
def test_model_restatement_error_is_neither_zero_nor_large(num_layers, hops):
    _, e32 = cases.model_expectation(num_layers, hops)
    assert 0 < e32 < 1e-4, e32


def test_chunked_restatement_is_the_mean_within_rounding_and_depends_on_the_order():
    """The bit-for-bit restatement of the documented order computes the layer (against float64), and chunking is visible in its bits: the
    hub rows differ from a plain slot-order sum somewhere, so the GPU test that pins the bits pins CHUNK too."""
    g = cases.graph("main")
    x = cases.layer_inputs(cases.LayerCase("main", 12, 7, False))["x"][:, :4].copy()
    got = cases.chunked_restatement(g, x, x)
    want = _dense_mean(g) @ torch.from_numpy(x).double() + torch.from_numpy(x).double()
    assert cases.err(got, want) < 1e-5
    hub = g.special[2 * cases.CHUNK + 1]
    plain = np.zeros(4, dtype=np.float32)
    for q in range(g.rowptr[hub], g.rowptr[hub + 1]):
        plain = plain + x[g.col[q]]
    plain = (plain * (np.float32(1) / np.float32(2 * cases.CHUNK + 1))).astype(np.float32) + x[hub]
    assert not np.array_equal(plain.view(np.uint32), got[hub].view(np.uint32))


def test_inference_on_cpu_tensors_raises_the_gpu_only_error():
    from graphpope_amd import sage
    g = cases.graph("main")
    model = sage.SAGE(cases.MODEL_IN, cases.MODEL_OUT, cases.MODEL_HIDDEN, 2)
    adj = sage.SampledAdj(torch.from_numpy(g.rowptr), torch.from_numpy(g.col), g.n)
    with pytest.raises(RuntimeError, match=r"GPU only \(no CPU fallback\)"):
        model.inference(torch.from_numpy(cases.model_x()), adj)
    with pytest.raises(ValueError, match="hops"):
        model.inference(torch.from_numpy(cases.model_x()), adj, hops=3)        # two convs: there is no third hop


def test_size_query_needs_no_device_and_refuses_what_does_not_fit(lib):
    q = lib.sage_full_layer_scratch_size
    flickr = q(89250, 899756, 756, 256)
    # stacked weights, the projected rows P | R and the hub partials, each rounded up to 256 bytes
    assert flickr >= 4 * (2 * 256 * 756 + 89250 * 512) and flickr < 4 * (2 * 256 * 756 + 89250 * 512) + 4 * 256 * (2 * 899756 // 512 + 8) + 8 * 256 + 64 * 1024
    assert flickr % 256 == 0 and q(1, 0, 36, 256) > 0
    assert q(300, 2000, 36, 256) > q(300, cases.CHUNK, 36, 256)            # room for hubs only where a row can be one
    i32 = 2 ** 31 - 1
    for bad in ((0, 0, 36, 256), (-1, 0, 36, 256), (i32, 10, 36, 256), (10, i32, 36, 256), (10, -1, 36, 256), (10, 10, 0, 256), (10, 10, 36, 0),
                (10, 10, 36, -4), (10, 10, 36, 2 ** 30)):
        assert q(*bad) == 0, bad
    big = q(1 << 22, 1 << 26, 756, 256)                                # R-MAT-22: N * 2 c_out is past 2^31 elements, sizes stay 64-bit
    assert big > 4 * (1 << 22) * 512 > 2 ** 32


def test_size_query_never_drops_while_an_argument_doubles(lib):
    """Each argument doubled from a small base up to the call's limit, the others fixed: the answer never drops and never becomes 0 -- a
    32-bit product that wrapped on the way would show as a drop (the sweep tests/test_workspace_cpu.py runs over the *_scratch_bytes
    queries)."""
    q = lib.sage_full_layer_scratch_size
    base, limits = (17, 1, 4, 4), (2 ** 31 - 2, 2 ** 31 - 2, 2 ** 31 - 2, 2 ** 30 - 1)
    for i, limit in enumerate(limits):
        args, prev, steps = list(base), q(*base), 0
        assert prev > 0
        while args[i] * 2 <= limit:
            args[i] *= 2
            now = q(*args)
            assert now >= prev and now > 0, (tuple(args), prev, now)
            prev, steps = now, steps + 1
        assert steps >= 15 and prev < 2 ** 62


def _forward(lib, **over):
    """sage_full_layer_forward on fake (never dereferenced) pointers: validation happens before anything touches the device."""
    a = dict(rowptr=64, col=64, N=10, nnz=20, x=64, c_in=8, w_l=64, b_l=64, w_r=64, c_out=8, gamma=0, beta=0, mean=0, var=0, eps=1e-5, out=64,
             scratch=64, scratch_bytes=1 << 30, stream=0)
    a.update(over)
    p = ctypes.c_void_p
    return lib.sage_full_layer_forward(p(a["rowptr"]), p(a["col"]), a["N"], a["nnz"], p(a["x"]), a["c_in"], p(a["w_l"]), p(a["b_l"]), p(a["w_r"]),
                                       a["c_out"], p(a["gamma"]), p(a["beta"]), p(a["mean"]), p(a["var"]), a["eps"], p(a["out"]), p(a["scratch"]),
                                       a["scratch_bytes"], p(a["stream"]))


def test_argument_validation_needs_no_device(lib):
    from graphpope_amd import _lib
    for name in ("rowptr", "col", "x", "w_l", "w_r", "out", "scratch"):
        assert _forward(lib, **{name: 0}) == _lib.ERR_INVALID, name
        assert b"null pointer" in lib.pope_last_error()
    i32 = 2 ** 31 - 1
    for over in (dict(N=i32), dict(N=0), dict(nnz=i32), dict(nnz=-1), dict(c_out=0), dict(c_out=-8), dict(c_in=0), dict(c_out=2 ** 30)):
        assert _forward(lib, **over) == _lib.ERR_INVALID, over
        assert b"bad size" in lib.pope_last_error()
    for given in (("gamma",), ("gamma", "beta"), ("gamma", "beta", "mean"), ("var",), ("beta", "mean", "var")):
        assert _forward(lib, **{k: 64 for k in given}) == _lib.ERR_INVALID, given
        assert b"go together" in lib.pope_last_error()
    need = lib.sage_full_layer_scratch_size(10, 20, 8, 8)
    assert _forward(lib, scratch_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert str(need).encode() in lib.pope_last_error()


def _name(lib, n, nnz, c_in, c_out, has_bn, mask=0, cap=384):
    from graphpope_amd import _lib
    buf = ctypes.create_string_buffer(cap)
    _lib.check(lib.sage_full_layer_kernel_name(n, nnz, c_in, c_out, has_bn, cases.CUS, mask, buf, cap))
    return buf.value.decode()


def test_kernel_name_prints_the_launch_list(lib):
    from graphpope_amd import _lib
    hub_t = "+k_full_hub_partial<true>+k_full_hub_finish<true, true>"
    # the product's layer 0 on the Flickr-shaped graph: whole tiles, 16-byte accesses, the hub launches
    assert _name(lib, 89250, 899756, 756, 256, 1) == "k_full_prepare+k_gemm_tile16<8, 4>+k_full_aggregate<true, true>" + hub_t
    # x misaligned: the plain tile kernel in its generic layout, the aggregate kernels stay vectorised (they read scratch, not x)
    assert _name(lib, 89250, 899756, 756, 256, 1, 1) == "k_full_prepare+k_gemm<128, 256, 4, 1, 0, 0>+k_full_aggregate<true, true>" + hub_t
    # out or scratch misaligned: the scalar aggregate kernels
    for mask in (2, 4, 7):
        assert _name(lib, 89250, 899756, 756, 256, 1, mask).endswith(
            "+k_full_aggregate<false, true>+k_full_hub_partial<false>+k_full_hub_finish<false, true>"), mask
    g = cases.graph("main")
    want = {(36, 256): "k_gemm<64, 64, 2, 2, 1, 1>", (36, 260): "k_gemm<64, 64, 2, 2, 1, 1>", (12, 7): "k_gemm<64, 64, 2, 2, 1, 1>",
            (256, 512): "k_gemm_tile16<1, 4>", (37, 64): "k_gemm<64, 64, 2, 2, 0, 0>"}        # depth 37: the generic GEMM fallback
    for (c_in, c_out), gemm in want.items():
        v = "true" if c_out % 4 == 0 else "false"
        assert _name(lib, g.n, g.nnz, c_in, c_out, 0) == \
            f"k_full_prepare+{gemm}+k_full_aggregate<{v}, false>+k_full_hub_partial<{v}>+k_full_hub_finish<{v}, false>", (c_in, c_out)
    assert _name(lib, 17, 0, 36, 256, 1) == "k_full_prepare+k_gemm<64, 64, 2, 2, 1, 1>+k_full_aggregate<true, true>"     # no row can be a hub
    assert _name(lib, 300, cases.CHUNK, 36, 256, 0).endswith("k_full_aggregate<true, false>")
    assert "k_full_hub_partial" in _name(lib, 300, cases.CHUNK + 1, 36, 256, 0)
    buf = ctypes.create_string_buffer(384)
    for bad in ((0, 0, 36, 256, 0, 256, 0), (300, 10, 36, 256, 0, 0, 0), (300, 10, 36, 256, 0, 256, 8), (2 ** 31 - 1, 10, 36, 256, 0, 256, 0)):
        assert lib.sage_full_layer_kernel_name(*bad, buf, 384) == _lib.ERR_INVALID, bad
    assert lib.sage_full_layer_kernel_name(300, 10, 36, 256, 0, 256, 0, None, 384) == _lib.ERR_INVALID
    assert lib.sage_full_layer_kernel_name(300, 10, 36, 256, 0, 256, 0, buf, 16) == _lib.ERR_INVALID and b"do not fit" in lib.pope_last_error()


def test_header_documents_the_chunk_and_cites_the_reference_lines():
    text = (ROOT / "include" / "graphpope_hip.h").read_text()
    assert int(re.search(r"CHUNK = (\d+)", text).group(1)) == cases.CHUNK
    source = (ROOT / "graphpope_amd" / "csrc" / "sage_full.h").read_text()
    assert int(re.search(r"constexpr int FULL_CHUNK = (\d+);", source).group(1)) == cases.CHUNK
    for symbol in ("sage_full_layer_scratch_size", "sage_full_layer_forward", "sage_full_layer_kernel_name"):
        comment = re.search(r'((?://[^\n]*\n)+)extern "C" [^\n]*\b' + symbol + r"\(", source)
        assert comment and "main.py:204-211" in comment.group(1), symbol
    assert text.count("main.py:204-211") >= 3


def test_command_line_keeps_the_reference_flag_surface():
    from graphpope_amd import main as cli
    flags = sorted(a.option_strings[0] for a in cli.build_parser()._actions if a.option_strings and a.option_strings[0] != "-h")
    assert flags == sorted(["--dataset", "--embedding_space", "--sampling_method", "--num_anchor_nodes", "--distance_function", "--num_workers",
                            "--dropout", "--lr", "--num_layers", "--hidden_layer_size", "--batch_size", "--epochs", "--seed", "--wandb_logging",
                            "--n_gpus"])
    assert len(flags) == 15
