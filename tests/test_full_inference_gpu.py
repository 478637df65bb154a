"""Exact full-graph SAGE inference on the GPU, through tests/full_inference_cases.py: sage_full_layer_forward on every layer case within
the threshold the float32 restatement sets, its bits (two calls, and the documented summation order restated in NumPy), SAGE.inference
and the existing eval path model.eval()(x, adjs) against the same float64 reference, operands that are not 16-byte aligned, the
scratch promise, and the command line's GRAPHPOPE_FULL_INFERENCE report."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import full_inference_cases as cases
import misaligned
from workspace import GuardedScratch, dev, lib  # noqa: F401  (the fixtures live in the helper module)

pytestmark = pytest.mark.gpu

SENTINEL = misaligned.SENTINEL


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    """A fault is sticky: every later call in the process would fail the same way.  The run ends at the test that met it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the GPU reported an error, nothing more is started: %s" % e, returncode=3)


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _graph_on(dev, g):
    return torch.from_numpy(g.rowptr).to(dev), torch.from_numpy(g.col).to(dev) if g.nnz else None


def _layer_call(lib, g, rowptr, col, t, c_in, c_out, out, scratch_ptr, scratch_bytes):
    """The raw call; t: name -> device tensor (gamma / beta / mean / var absent: no BatchNorm)."""
    return lib.sage_full_layer_forward(_ptr(rowptr), _ptr(col), g.n, g.nnz, _ptr(t["x"]), c_in, _ptr(t["w_l"]), _ptr(t.get("b_l")), _ptr(t["w_r"]),
                                       c_out, _ptr(t.get("gamma")), _ptr(t.get("beta")), _ptr(t.get("mean")), _ptr(t.get("var")), cases.EPS,
                                       _ptr(out), scratch_ptr, scratch_bytes, _stream())


def _run_layer(lib, dev, g, arrays, c_in, c_out):
    """sage_full_layer_forward on aligned operands and a scratch of the queried size: the result on the host."""
    from graphpope_amd import _lib
    rowptr, col = _graph_on(dev, g)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in arrays.items()}
    out = torch.full((g.n, c_out), SENTINEL, dtype=torch.float32, device=dev)
    nbytes = lib.sage_full_layer_scratch_size(g.n, g.nnz, c_in, c_out)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(_layer_call(lib, g, rowptr, col, t, c_in, c_out, out, _ptr(scratch), nbytes))
    return out.cpu()


def _report(what, got, want64, limit):
    e = cases.err(got, want64)
    print(f"{what}: err {e:.3e} limit {limit:.3e}")
    return e


@pytest.mark.parametrize("case", cases.LAYER_CASES, ids=lambda c: c.id)
def test_entry_point_within_the_threshold(lib, dev, case):
    want, _ = cases.layer_expectation(case)
    got = _run_layer(lib, dev, cases.graph(case.graph), cases.layer_inputs(case), case.c_in, case.c_out)
    assert torch.isfinite(got).all()
    limit = cases.layer_threshold(case)
    assert _report(case.id, got, want, limit) <= limit
    again = _run_layer(lib, dev, cases.graph(case.graph), cases.layer_inputs(case), case.c_in, case.c_out)
    assert got.numpy().tobytes() == again.numpy().tobytes()               # two calls, equal bits


def test_chunk_is_the_documented_value():
    text = (Path(__file__).resolve().parents[1] / "include" / "graphpope_hip.h").read_text()
    assert int(re.search(r"CHUNK = (\d+)", text).group(1)) == cases.CHUNK


@pytest.mark.parametrize("c, has_bn", [(1, False), (4, False), (4, True), (260, False)])
def test_bits_of_the_documented_order(lib, dev, c, has_bn):
    """c_in = c_out = c with identity weights and no bias: the projection is exact (P = R = x), so every row -- the hub rows among them --
    must carry the bits of the NumPy float32 restatement of the documented order (c = 1: the scalar kernels, 4: the 16-byte ones, 260: two
    slabs)."""
    g = cases.graph("main")
    rs = np.random.RandomState(90 + c)
    arrays = {"x": rs.randn(g.n, c).astype(np.float32), "w_l": np.eye(c, dtype=np.float32), "w_r": np.eye(c, dtype=np.float32),
              "b_l": np.zeros(c, dtype=np.float32)}
    bn = None
    if has_bn:
        b = cases._bn_arrays(rs, c)
        arrays.update(b)
        bn = (b["gamma"], b["beta"], b["mean"], b["var"])
    got = _run_layer(lib, dev, g, arrays, c, c).numpy()
    want = cases.chunked_restatement(g, arrays["x"], arrays["x"], bn)
    for d in cases.DEGREES:
        v = g.special[d]
        assert np.array_equal(got[v].view(np.uint32), want[v].view(np.uint32)), (d, got[v][:4], want[v][:4])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ models

def _model(dev, num_layers):
    from graphpope_amd import sage
    model = sage.SAGE(cases.MODEL_IN, cases.MODEL_OUT, cases.MODEL_HIDDEN, num_layers)
    model.load_state_dict(cases.model_state(num_layers))
    return model.to(dev)


@pytest.mark.parametrize("num_layers, hops", cases.MODELS)
@pytest.mark.parametrize("adjacency", ["SampledAdj", "Csr"])
def test_inference_within_the_threshold(dev, num_layers, hops, adjacency):
    from graphpope_amd import engine, sage
    g = cases.graph("main")
    model = _model(dev, num_layers).train()                                  # running statistics whatever self.training says
    if adjacency == "Csr":
        adj = engine.build_csr(torch.from_numpy(np.stack([g.dst, g.src])).to(dev), g.n)        # row v of the CSR: v's slots (any order)
    else:
        rowptr, col = _graph_on(dev, g)
        adj = sage.SampledAdj(rowptr, col, g.n)
    x = torch.from_numpy(cases.model_x()).to(dev)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    got = model.inference(x, adj, hops=hops)
    want, _ = cases.model_expectation(num_layers, hops)
    assert got.shape == want.shape and got.dtype == torch.float32 and not got.requires_grad and model.training
    limit = cases.model_threshold(num_layers, hops)
    assert _report(f"inference {num_layers}/{hops} {adjacency}", got.cpu(), want, limit) <= limit
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())               # nothing of the model moved
    if hops == num_layers:
        assert torch.equal(model.inference(x, adj), got)                     # the default depth: every conv


@pytest.mark.parametrize("num_layers, hops", cases.MODELS)
def test_existing_eval_path_meets_the_same_threshold(dev, num_layers, hops):
    """model.eval()(x, adjs) with blocks that take every neighbour -- all nodes as seeds, so each block is the whole CSR -- against the same
    float64 reference and the same threshold: the new path and what training runs compute the same function, depth quirk included."""
    from graphpope_amd import sage
    g = cases.graph("main")
    model = _model(dev, num_layers).eval()
    rowptr, col = _graph_on(dev, g)
    adjs = [sage.SampledAdj(rowptr, col, g.n) for _ in range(hops)]
    with torch.no_grad():
        got = model(torch.from_numpy(cases.model_x()).to(dev), adjs)
    want, _ = cases.model_expectation(num_layers, hops)
    limit = cases.model_threshold(num_layers, hops)
    assert got.shape == want.shape
    assert _report(f"eval path {num_layers}/{hops}", got.cpu(), want, limit) <= limit


# ------------------------------------------------------------------------------------------------ alignment and scratch

@pytest.mark.parametrize("operand", ["x", "w_l", "w_r", "out", "scratch", "all"])
@pytest.mark.parametrize("case", [cases.LayerCase("main", 36, 256, True), cases.LayerCase("main", 256, 512, False)], ids=lambda c: c.id)
def test_misaligned_operands(lib, dev, case, operand):
    """Each operand in turn (and all of them) 4 bytes past a 16-byte boundary: the values stay within the threshold and no float in front
    of or behind a view is touched."""
    from graphpope_amd import _lib
    g, arrays = cases.graph(case.graph), cases.layer_inputs(case)
    off = lambda name: 1 if operand in (name, "all") else 0               # noqa: E731
    rowptr, col = _graph_on(dev, g)
    t = {k: misaligned.place(v, dev, off(k)) for k, v in arrays.items()}
    out = misaligned.place(np.full((g.n, case.c_out), SENTINEL), dev, off("out"))
    nbytes = lib.sage_full_layer_scratch_size(g.n, g.nnz, case.c_in, case.c_out)
    assert nbytes % 4 == 0
    scratch = misaligned.place(np.full(nbytes // 4, SENTINEL), dev, off("scratch"))
    _lib.check(_layer_call(lib, g, rowptr, col, t, case.c_in, case.c_out, out, _ptr(scratch), nbytes))
    got = out.cpu()
    want, _ = cases.layer_expectation(case)
    limit = cases.layer_threshold(case)
    assert _report(f"{case.id} misaligned {operand}", got, want, limit) <= limit
    for name, view in (*t.items(), ("out", out), ("scratch", scratch)):
        assert misaligned.guards_intact(view), name
    for k, v in arrays.items():
        assert np.array_equal(t[k].cpu().numpy(), v), k                    # inputs are read only


@pytest.mark.parametrize("case", [cases.LayerCase("main", 36, 260, True), cases.LayerCase("main", 256, 512, False),
                                  cases.LayerCase("empty", 36, 256, True)], ids=lambda c: c.id)
def test_scratch_promise(lib, dev, case):
    """Exactly the queried bytes, full of 0xFF, between guard bands: the bands stay, the result is finite and has the bits of a call on
    fresh memory.  One byte less: POPE_ERR_WORKSPACE with the needed size, `out` untouched, not a byte of the buffer changed."""
    from graphpope_amd import _lib
    g, arrays = cases.graph(case.graph), cases.layer_inputs(case)
    rowptr, col = _graph_on(dev, g)
    t = {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
    nbytes = lib.sage_full_layer_scratch_size(g.n, g.nnz, case.c_in, case.c_out)
    guarded = GuardedScratch(dev, nbytes).fill("ones")
    out = torch.full((g.n, case.c_out), SENTINEL, dtype=torch.float32, device=dev)
    _lib.check(_layer_call(lib, g, rowptr, col, t, case.c_in, case.c_out, out, guarded.ptr, nbytes))
    assert guarded.bands_intact()
    assert torch.isfinite(out).all()
    assert out.cpu().numpy().tobytes() == _run_layer(lib, dev, g, arrays, case.c_in, case.c_out).numpy().tobytes()
    guarded.fill("ones")
    before = guarded.snapshot()
    out.fill_(SENTINEL)
    ptr, short = guarded.short(1)
    assert _layer_call(lib, g, rowptr, col, t, case.c_in, case.c_out, out, ptr, short) == _lib.ERR_WORKSPACE
    assert str(nbytes).encode() in lib.pope_last_error()
    assert bool((out == SENTINEL).all()) and guarded.unchanged_since(before)
    name = ctypes.create_string_buffer(384)                                   # a call that succeeds: no error message is left behind
    assert lib.sage_full_layer_kernel_name(g.n, g.nnz, case.c_in, case.c_out, int(case.has_bn), cases.CUS, 0, name, 384) == 0


# ------------------------------------------------------------------------------------------------ command line

def test_command_line_reports_full_graph_accuracy(capsys, monkeypatch, tmp_path, lib):
    """python -m graphpope_amd.main on the PubMed-shaped graph, one epoch, under GRAPHPOPE_DETERMINISTIC=1 with one seed: with
    GRAPHPOPE_FULL_INFERENCE=1 a full_val_acc / full_test_acc line in [0, 1] follows the test accuracy, and the value main() returns and
    every other line are those of the run without the variable."""
    from graphpope_amd import main as cli, utils as gp
    monkeypatch.setenv("GRAPHPOPE_DATA_DIR", str(tmp_path))                   # no pubmed.npz there: the synthetic PubMed-shaped graph
    monkeypatch.setenv("GRAPHPOPE_DETERMINISTIC", "1")
    argv = ["--dataset", "pubmed", "--embedding_space", "geodesic", "--sampling_method", "stochastic", "--num_anchor_nodes", "8",
            "--epochs", "1", "--seed", "11"]
    runs = {}
    for full in ("1", None):
        if full is None:
            monkeypatch.delenv("GRAPHPOPE_FULL_INFERENCE", raising=False)
        else:
            monkeypatch.setenv("GRAPHPOPE_FULL_INFERENCE", full)
        gp.clear_cache()
        capsys.readouterr()
        acc = cli.main(argv)
        runs[full] = (acc, capsys.readouterr().out.splitlines())
    gp.clear_cache()
    assert lib.sage_get_deterministic() == 0
    (acc_full, lines_full), (acc_plain, lines_plain) = runs["1"], runs[None]
    assert acc_full == acc_plain and 0.0 <= acc_plain <= 1.0
    assert lines_full[:-1] == lines_plain and lines_plain[-1].startswith("test_acc ")
    m = re.fullmatch(r"full_val_acc (\d\.\d{4}) full_test_acc (\d\.\d{4})", lines_full[-1])
    assert m, lines_full[-1]
    assert 0.0 <= float(m.group(1)) <= 1.0 and 0.0 <= float(m.group(2)) <= 1.0
