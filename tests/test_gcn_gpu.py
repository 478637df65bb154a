"""GCNConv / GCN on the GPU, through tests/gcn_cases.py: pope_gcn_degree_norm and pope_gcn_propagate bit for bit against the NumPy
restatement of the header's summation contract (both CSR directions, every flag, scalar and 16-byte forms, one and two slabs, operands
off the 16-byte grid, guarded and poisoned scratch, the refused short scratch); the layer and the two-layer model, out, loss and every
gradient, against the float64 dense formula within the rule; bit-reproducibility in both modes of the library; a training smoke test and
the command line."""
import ctypes
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import gcn_cases as cases
from conftest import ROOT
from workspace import GuardedScratch, dev, lib  # noqa: F401  (the fixtures live in the helper module)

pytestmark = pytest.mark.gpu


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


def _up(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def csrs(dev):
    """Device copies of both CSRs of every graph: {(name, by_source): (rowptr, col)}."""
    return {(name, t): tuple(_up(dev, a) for a in cases.csr(name, t)) for name in ("main", "single", "empty") for t in (False, True)}


@pytest.fixture(scope="module")
def dinvs(dev, lib, csrs):
    """pope_gcn_degree_norm on the by-destination CSR of the main graph, per self weight: the device vector the propagate tests use."""
    g = cases.graph("main")
    out = {}
    for f in (0.0, 1.0, 2.0):
        d = torch.empty(g.n, dtype=torch.float32, device=dev)
        rowptr, col = csrs["main", False]
        assert lib.pope_gcn_degree_norm(_ptr(rowptr), _ptr(col), g.n, g.nnz, f, _ptr(d), _stream()) == 0, lib.pope_last_error()
        out[f] = d
    return out


# ------------------------------------------------------------------------------------------------ the degree pass

@pytest.mark.parametrize("improved,add_self_loops", cases.SETTINGS)
def test_dinv_bit_for_bit(improved, add_self_loops, dinvs):
    g, f = cases.graph("main"), cases.self_weight(improved, add_self_loops)
    want = cases.dinv_restatement(g.rowptr, g.col, g.n, f)
    assert np.array_equal(_bits(dinvs[f].cpu().numpy()), _bits(want))


def test_dinv_of_the_degenerate_graphs(dev, lib, csrs):
    for name in ("single", "empty"):
        g = cases.graph(name)
        rowptr, col = csrs[name, False]
        for f, want in ((1.0, 1.0), (0.0, 0.0), (2.0, float(np.float32(1.0 / np.sqrt(2.0))))):
            d = torch.full((g.n,), 7.0, dtype=torch.float32, device=dev)
            assert lib.pope_gcn_degree_norm(_ptr(rowptr), _ptr(col), g.n, 0, f, _ptr(d), _stream()) == 0
            assert (d.cpu().numpy() == np.float32(want)).all()


# ------------------------------------------------------------------------------------------------ the propagate, bit for bit

# (dinv, self weight, bias)
FLAGS = ((True, 1.0, True), (True, 2.0, False), (True, 0.0, True), (False, 0.0, False), (False, 1.0, True))


def _rows(c):
    rs = np.random.RandomState(8000 + c)
    g = cases.graph("main")
    return (0.25 + rs.randn(g.n, c)).astype(np.float32), rs.randn(c).astype(np.float32)


def _propagate(dev, lib, rowptr, col, n, nnz, dinv, f, h, bias, offset=0, fill="noise"):
    """pope_gcn_propagate with `out` and the scratch between guard bands, the scratch exactly the queried size and poisoned beforehand;
    offset: every operand that many bytes off the 256-byte grid.  -> (out on the host, status)."""
    c = h.shape[1]
    nbytes = lib.pope_gcn_propagate_scratch_size(n, nnz, c)
    assert nbytes > 0
    scratch = GuardedScratch(dev, nbytes + offset).fill(fill)
    out = GuardedScratch(dev, n * c * 4 + offset).fill("ones")
    h_buf = torch.empty(n * c + 4, dtype=torch.float32, device=dev)
    h_dev = h_buf[offset // 4:offset // 4 + n * c].view(n, c)
    h_dev.copy_(torch.from_numpy(h))
    at = lambda gs: ctypes.c_void_p(gs.ptr.value + offset)                                              # noqa: E731
    rc = lib.pope_gcn_propagate(_ptr(rowptr), _ptr(col), n, nnz, _ptr(dinv), f, _ptr(h_dev), c, _ptr(bias), at(out), at(scratch), nbytes, _stream())
    torch.cuda.synchronize()
    assert scratch.bands_intact() and out.bands_intact()
    got = out.view[offset:offset + n * c * 4].cpu().numpy().copy().view(np.float32).reshape(n, c)
    return got, rc


@pytest.mark.parametrize("by_source", (False, True), ids=("by_dst", "by_src"))
@pytest.mark.parametrize("c", cases.PROPAGATE_WIDTHS)
def test_propagate_bit_for_bit(by_source, c, dev, lib, csrs, dinvs):
    g = cases.graph("main")
    rowptr, col = cases.csr("main", by_source)
    h, b = _rows(c)
    b_dev = _up(dev, b)
    for has_dinv, f, has_bias in FLAGS:
        dinv = cases.dinv_restatement(g.rowptr, g.col, g.n, f) if has_dinv else None       # by destination, for BOTH directions
        want = cases.propagate_restatement(rowptr, col, g.n, h, dinv, f, b if has_bias else None)
        got, rc = _propagate(dev, lib, *csrs["main", by_source], g.n, g.nnz, dinvs[f] if has_dinv else None, f, h, b_dev if has_bias else None)
        assert rc == 0, lib.pope_last_error()
        diff = _bits(got) != _bits(want)
        assert not diff.any(), (has_dinv, f, has_bias, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def test_propagate_off_the_16_byte_grid_gives_the_same_bits(dev, lib, csrs, dinvs):
    g = cases.graph("main")
    h, b = _rows(256)
    want = cases.propagate_restatement(g.rowptr, g.col, g.n, h, cases.dinv_restatement(g.rowptr, g.col, g.n, 1.0), 1.0, b)
    b_buf = torch.zeros(257, dtype=torch.float32, device=dev)
    b_buf[1:].copy_(torch.from_numpy(b))
    got, rc = _propagate(dev, lib, *csrs["main", False], g.n, g.nnz, dinvs[1.0], 1.0, h, b_buf[1:], offset=4)
    assert rc == 0, lib.pope_last_error()
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("fill", ("zeros", "ones"))
def test_propagate_does_not_read_what_it_did_not_write(fill, dev, lib, csrs, dinvs):
    g = cases.graph("main")
    h, b = _rows(64)
    want = cases.propagate_restatement(g.rowptr, g.col, g.n, h, cases.dinv_restatement(g.rowptr, g.col, g.n, 1.0), 1.0, None)
    got, rc = _propagate(dev, lib, *csrs["main", False], g.n, g.nnz, dinvs[1.0], 1.0, h, None, fill=fill)
    assert rc == 0 and np.array_equal(_bits(got), _bits(want))


def test_a_scratch_one_byte_short_is_refused_and_nothing_is_written(dev, lib, csrs, dinvs):
    from graphpope_amd import _lib
    g = cases.graph("main")
    h, _ = _rows(64)
    rowptr, col = csrs["main", False]
    nbytes = lib.pope_gcn_propagate_scratch_size(g.n, g.nnz, 64)
    scratch = GuardedScratch(dev, nbytes).fill("noise")
    out = GuardedScratch(dev, g.n * 64 * 4).fill("noise")
    before, before_out = scratch.snapshot(), out.snapshot()
    ptr, short = scratch.short(1)
    rc = lib.pope_gcn_propagate(_ptr(rowptr), _ptr(col), g.n, g.nnz, _ptr(dinvs[1.0]), 1.0, _ptr(_up(dev, h)), 64, None, out.ptr, ptr, short, _stream())
    assert rc == _lib.ERR_WORKSPACE and str(nbytes).encode() in lib.pope_last_error()
    assert scratch.unchanged_since(before) and out.unchanged_since(before_out)
    for query, call_args in ((lib.pope_gcn_conv_forward_scratch_size, "forward"), (lib.pope_gcn_conv_backward_scratch_size, "backward")):
        need = query(g.n, g.nnz, 36, 64)
        s = GuardedScratch(dev, need).fill("noise")
        snap = s.snapshot()
        x, w, o = (torch.zeros(n, dtype=torch.float32, device=dev) for n in (g.n * 36, 36 * 64, g.n * 64))
        if call_args == "forward":
            rc = lib.pope_gcn_conv_forward(_ptr(rowptr), _ptr(col), g.n, g.nnz, _ptr(dinvs[1.0]), 1.0, _ptr(x), 36, _ptr(w), None, 64, _ptr(o), s.ptr,
                                           need - 1, _stream())
        else:
            rc = lib.pope_gcn_conv_backward(_ptr(rowptr), _ptr(col), g.n, g.nnz, _ptr(dinvs[1.0]), 1.0, _ptr(x), 36, _ptr(w), 64, _ptr(o), None,
                                            _ptr(torch.zeros_like(w)), None, s.ptr, need - 1, _stream())
        assert rc == _lib.ERR_WORKSPACE and s.unchanged_since(snap), call_args


def test_empty_rows_with_unit_self_weight_return_h_plus_b(dev, lib, csrs):
    for name in ("empty", "single"):
        g = cases.graph(name)
        rs = np.random.RandomState(9)
        h, b = rs.randn(g.n, 260).astype(np.float32), rs.randn(260).astype(np.float32)
        rowptr, col = csrs[name, False]
        dinv = torch.empty(g.n, dtype=torch.float32, device=dev)
        assert lib.pope_gcn_degree_norm(_ptr(rowptr), _ptr(col), g.n, 0, 1.0, _ptr(dinv), _stream()) == 0
        got, rc = _propagate(dev, lib, rowptr, col, g.n, 0, dinv, 1.0, h, _up(dev, b))
        assert rc == 0 and np.array_equal(_bits(got), _bits(h + b))


# ------------------------------------------------------------------------------------------------ the layer against float64

@pytest.fixture(scope="module")
def adj(dev):
    from graphpope_amd import gcn
    g = cases.graph("main")
    return gcn.GraphAdj(torch.from_numpy(np.stack([g.src, g.dst])).to(dev), g.n)


def test_graph_adj_builds_both_canonical_csrs(adj):
    g = cases.graph("main")
    rowptr_t, col_t = cases.transposed("main")
    assert np.array_equal(adj.rowptr_t.cpu().numpy(), rowptr_t) and np.array_equal(adj.col_t.cpu().numpy()[:g.nnz], col_t)
    assert np.array_equal(adj.rowptr.cpu().numpy(), g.rowptr)
    col = adj.col.cpu().numpy()
    for i in range(g.n):                                               # the same rows as the test graph's, each ascending
        assert np.array_equal(col[g.rowptr[i]:g.rowptr[i + 1]], np.sort(g.col[g.rowptr[i]:g.rowptr[i + 1]]))
    assert adj.dinv(True, False) is adj.dinv(False, False) and adj.dinv() is adj.dinv(False, True)      # cached per (f, self loops)
    assert np.array_equal(_bits(adj.dinv(True, True).cpu().numpy()), _bits(cases.dinv_restatement(g.rowptr, g.col, g.n, 2.0)))


def _device_layer(dev, adj, case):
    from graphpope_amd import gcn
    t = cases.layer_inputs(case)
    conv = gcn.GCNConv(case.c_in, case.c_out, improved=case.improved, add_self_loops=case.add_self_loops, normalize=case.normalize,
                       bias=case.bias).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(t["weight"]))
        if case.bias:
            conv.bias.copy_(torch.from_numpy(t["bias"]))
    x = torch.from_numpy(t["x"]).to(dev).requires_grad_(case.grad_x)
    out = conv(x, adj)
    (out * torch.from_numpy(t["g"]).to(dev)).sum().backward()
    got = {"out": out.detach().cpu(), "grad_weight": conv.weight.grad.cpu()}
    if case.grad_x:
        got["grad_x"] = x.grad.cpu()
    if case.bias:
        got["grad_bias"] = conv.bias.grad.cpu()
    return got


@pytest.mark.parametrize("case", cases.LAYER_CASES, ids=lambda c: c.id)
def test_layer_out_and_every_gradient_within_the_rule(case, dev, lib, adj):
    g = cases.graph("main")
    name = ctypes.create_string_buffer(512)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert lib.pope_gcn_kernel_name(g.n, g.nnz, case.c_in, case.c_out, 0, 1, cus, 0, name, 512) == 0
    whole = (case.c_in, case.c_out) == cases.WHOLE_TILE_SHAPE
    assert ("k_gemm_tile16<" in name.value.decode()) == whole and ("k_gemm<" in name.value.decode()) == (not whole), name.value
    t64, err32 = cases.layer_expectation(case)
    got = _device_layer(dev, adj, case)
    assert set(got) == set(t64) - (set() if case.grad_x else {"grad_x"})
    report = {k: (cases.err(got[k], t64[k]), cases.threshold(err32[k])) for k in got}
    print(case.id, {k: "%.3g / %.3g" % v for k, v in report.items()})
    for k, (e, bound) in report.items():
        assert e <= bound, (k, e, bound)


# ------------------------------------------------------------------------------------------------ the model

def _device_model(dev, adj, dropout=0.0):
    from graphpope_amd import gcn
    t = cases.model_inputs()
    model = gcn.GCN(cases.MODEL_IN, cases.MODEL_HIDDEN, cases.MODEL_OUT, num_layers=2, dropout=dropout).to(dev)
    model.load_state_dict({k: torch.from_numpy(t[k]) for k in cases.PARAMS})
    return model, torch.from_numpy(t["x"]).to(dev), torch.from_numpy(t["y"]).to(dev)


def _model_step(model, x, y, adj):
    from graphpope_amd import sage
    seen = []
    hook = model.convs[0].register_forward_hook(lambda m, i, o: seen.append(o.detach()))
    for p in model.parameters():
        p.grad = None
    logits = model(x, adj)
    loss = sage.cross_entropy(logits, y)
    loss.backward()
    hook.remove()
    got = {"logits": logits.detach().cpu(), "loss": float(loss.detach()), "z": seen[0].cpu()}
    got.update({"grad:" + k: p.grad.cpu() for k, p in model.named_parameters()})
    return got


def test_two_layer_model_loss_and_every_gradient(dev, adj):
    model, x, y = _device_model(dev, adj)
    got = _model_step(model, x, y, adj)
    ref, err32, gated, mismatches = cases.model_expectation(got["z"] > 0)
    assert gated <= cases.EXCLUDED_CAP * got["z"].numel() and mismatches == 0, (gated, mismatches)
    report = {k: (cases.err(got[k], ref[k]), cases.threshold(err32[k])) for k in err32}
    print({k: "%.3g / %.3g" % v for k, v in report.items()}, "loss", abs(got["loss"] - ref["loss"]), cases.loss_bound(ref, err32))
    for k, (e, bound) in report.items():
        assert e <= bound, (k, e, bound)
    assert abs(got["loss"] - ref["loss"]) <= cases.loss_bound(ref, err32)


def test_forward_and_backward_are_bit_reproducible_in_both_modes(dev, adj):
    from graphpope_amd import sage
    model, x, y = _device_model(dev, adj)
    runs = []
    for mode in (False, False, True, True):
        with sage.deterministic(mode):
            got = _model_step(model, x, y, adj)
        runs.append({k: _bits(v.numpy()) for k, v in got.items() if k != "loss"})
    for other in runs[1:]:
        for k, bits in runs[0].items():
            assert np.array_equal(bits, other[k]), k


def test_training_smoke(dev):
    """A planted-partition graph, 30 full-batch steps at dropout 0.5 through the product's loss and optimiser: the loss falls and every
    parameter stays finite."""
    from graphpope_amd import gcn, optim, sage
    ei, x, y = cases.planted_partition()
    torch.manual_seed(3)
    adj = gcn.GraphAdj(torch.from_numpy(ei).to(dev), x.shape[0])
    model = gcn.GCN(16, 32, 3, num_layers=2, dropout=0.5).to(dev)
    opt = optim.Adam(model.parameters(), lr=0.02, max_grad_norm=0.5)
    x, y = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    losses = []
    model.train()
    for _ in range(30):
        for p in model.parameters():
            p.grad = None
        loss = sage.cross_entropy(model(x, adj), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < 0.8 * np.mean(losses[:5]), losses
    model.eval()
    with torch.no_grad():
        acc = float((model(x, adj).argmax(-1) == y).float().mean())
    assert acc > 0.6, acc


def test_command_line_trains_a_gcn(tmp_path):
    """GRAPHPOPE_MODEL=gcn python -m graphpope_amd.main --dataset pubmed --epochs 2 --num_layers 2 in a child process (the synthetic
    PubMed-shaped graph): exit 0, the note about --batch_size, two epoch lines and a test_acc line at the end."""
    env = dict(os.environ, GRAPHPOPE_MODEL="gcn", GRAPHPOPE_DATA_DIR=str(tmp_path))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "graphpope_amd.main", "--dataset", "pubmed", "--epochs", "2", "--num_layers", "2"]
    proc = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, errs = proc.communicate(timeout=240.0)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.communicate()
        pytest.fail("GRAPHPOPE_MODEL=gcn python -m graphpope_amd.main did not finish within 240 s")
    assert proc.returncode == 0, errs[-4000:]
    lines = [line for line in out.splitlines() if line.strip()]
    assert any("--batch_size" in line and "unused" in line for line in lines)
    assert [line.split(":")[0] for line in lines if line.startswith("epoch ")] == ["epoch 0", "epoch 1"]
    assert lines[-1].startswith("test_acc ") and 0.0 <= float(lines[-1].split()[1]) <= 1.0
