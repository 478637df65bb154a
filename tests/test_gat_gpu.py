"""GATConv / GAT on the GPU, through tests/gat_cases.py: the slot map against its restatement; the scores bit for bit; the attention
within the rule; the propagate, given the device's own alpha, bit for bit against the NumPy restatement of the header's summation contract
(both concat settings, hub rows, scalar and 16-byte forms, two slabs, off the 16-byte grid, guarded and poisoned buffers, the refused
short scratch); the layer and the two-layer model, out, loss and every gradient, against the float64 dense formula within the rule under
the LeakyReLU gate; bit-reproducibility in both modes of the library; a training smoke test and the command line."""
import ctypes
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import gat_cases as cases
from conftest import ROOT
from workspace import GuardedScratch, dev, lib  # noqa: F401  (the fixtures live in the helper module)

pytestmark = pytest.mark.gpu

HEAD_SHAPES = ((1, 64), (4, 64), (8, 8), (3, 7), (2, 130), (1, 5))


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
    """Device copies of the canonical CSRs of every graph: {(name, by_source): (rowptr, col)}."""
    return {(name, t): tuple(_up(dev, a) for a in cases.canonical(name, t)) for name in ("main", "single", "empty") for t in (False, True)}


@pytest.fixture(scope="module")
def adj(dev):
    from graphpope_amd import gcn
    g = cases.graph("main")
    return gcn.GraphAdj(torch.from_numpy(np.stack([g.src, g.dst])).to(dev), g.n)


# ------------------------------------------------------------------------------------------------ the slot map

def test_slot_map_equals_the_restatement(dev, lib, csrs, adj):
    g = cases.graph("main")
    want = cases.slot_map_restatement("main")
    out = GuardedScratch(dev, g.nnz * 4).fill("ones")
    (rowptr, col), (rowptr_t, col_t) = csrs["main", False], csrs["main", True]
    assert lib.pope_gat_slot_map(_ptr(rowptr), _ptr(col), _ptr(rowptr_t), _ptr(col_t), g.n, g.nnz, out.ptr, _stream()) == 0, lib.pope_last_error()
    torch.cuda.synchronize()
    assert out.bands_intact() and np.array_equal(out.view.cpu().numpy().view(np.int32), want)
    assert adj.slot_map is adj.slot_map and np.array_equal(adj.slot_map.cpu().numpy()[:g.nnz], want)      # built once, kept
    assert np.array_equal(adj.col.cpu().numpy()[:g.nnz], cases.canonical("main", False)[1])


# ------------------------------------------------------------------------------------------------ scores and attention

def _heads_inputs(H, C, scale=1.0):
    g = cases.graph("main")
    rs = np.random.RandomState(8100 + 31 * H + C)
    return ((0.25 + rs.randn(g.n, H, C)).astype(np.float32), (scale * rs.randn(H, C) / np.sqrt(C)).astype(np.float32),
            (scale * rs.randn(H, C) / np.sqrt(C)).astype(np.float32), rs.randn(H * C).astype(np.float32))


def _attention(dev, lib, csr, n, nnz, h, att_l, att_r, slope, self_loops, fill="ones"):
    """pope_gat_attention with every output between guard bands and poisoned beforehand -> (a_src, a_dst, alpha, alpha_self) on the host."""
    H = h.shape[1]
    bufs = [GuardedScratch(dev, size * 4).fill(fill) for size in (n * H, n * H, nnz * H, n * H)]
    h_dev, l_dev, r_dev = _up(dev, h), _up(dev, att_l), _up(dev, att_r)            # (named: they live until the call has run)
    rc = lib.pope_gat_attention(_ptr(csr[0]), _ptr(csr[1]), n, nnz, _ptr(h_dev), H, h.shape[2], _ptr(l_dev), _ptr(r_dev),
                                slope, int(self_loops), *(b.ptr for b in bufs), _stream())
    assert rc == 0, lib.pope_last_error()
    torch.cuda.synchronize()
    assert all(b.bands_intact() for b in bufs)
    shapes = ((n, H), (n, H), (nnz, H), (n, H))
    return tuple(b.view.cpu().numpy().copy().view(np.float32).reshape(s) for b, s in zip(bufs, shapes))


def _alpha_in(dtype, rowptr, col, n, a_src, a_dst, slope, self_loops):
    """The attention of every slot and of the self term from the scores, row by row in `dtype` (max, exp, sum, divide)."""
    a_src, a_dst = a_src.astype(dtype), a_dst.astype(dtype)
    alpha, own = np.zeros((col.size, a_src.shape[1]), dtype=dtype), np.zeros_like(a_src)
    for i in range(n):
        ids = col[rowptr[i]:rowptr[i + 1]]
        term = (ids != i) if self_loops else np.ones(ids.size, dtype=bool)
        e = a_src[np.concatenate([ids[term], [i]]) if self_loops else ids[term]] + a_dst[i][None]
        if e.shape[0] == 0:
            continue
        e = np.where(e > 0, e, dtype(slope) * e)
        ex = np.exp(e - e.max(0, keepdims=True))
        w = (ex / ex.sum(0, keepdims=True)).astype(dtype)
        block = alpha[rowptr[i]:rowptr[i + 1]]
        block[term] = w[:int(term.sum())]
        if self_loops:
            own[i] = w[-1]
    return alpha, own


@pytest.mark.parametrize("H,C", HEAD_SHAPES)
def test_scores_bit_for_bit_and_alpha_within_the_rule(H, C, dev, lib, csrs):
    g = cases.graph("main")
    rowptr, col = cases.canonical("main", False)
    rows = np.repeat(np.arange(g.n), np.diff(rowptr))
    h, att_l, att_r, _ = _heads_inputs(H, C)
    for self_loops, slope in ((True, 0.2), (False, 0.2), (True, 0.0)):
        a_src, a_dst, alpha, alpha_self = _attention(dev, lib, csrs["main", False], g.n, g.nnz, h, att_l, att_r, slope, self_loops)
        assert np.array_equal(_bits(a_src), _bits(cases.scores_restatement(h, att_l)))
        assert np.array_equal(_bits(a_dst), _bits(cases.scores_restatement(h, att_r)))
        # the reference and the float32 draw both start from the device's scores: what is tested is the softmax
        want, want_self = _alpha_in(np.float64, rowptr, col, g.n, a_src, a_dst, slope, self_loops)
        draw, draw_self = _alpha_in(np.float32, rowptr, col, g.n, a_src, a_dst, slope, self_loops)
        bound = cases.threshold(max(cases.err(draw, want), cases.err(draw_self, want_self) if self_loops else 0.0))
        print((H, C, self_loops, slope), cases.err(alpha, want), bound)
        assert cases.err(alpha, want) <= bound and np.isfinite(alpha).all()
        if self_loops:
            assert cases.err(alpha_self, want_self) <= bound and (alpha[col == rows] == 0).all()
        else:
            assert (alpha_self == 0).all()
        total = np.zeros((g.n, H), dtype=np.float64)
        np.add.at(total, rows, alpha.astype(np.float64))
        total += alpha_self
        has_terms = np.ones(g.n, dtype=bool) if self_loops else np.diff(rowptr) > 0
        assert np.abs(total[has_terms] - 1).max() <= 4 * 2.0 ** -23 and (total[~has_terms] == 0).all()


# ------------------------------------------------------------------------------------------------ the propagate, bit for bit

def _propagate(dev, lib, csr, n, nnz, alpha, alpha_self, h, concat, bias, offset=0, fill="noise"):
    """pope_gat_propagate with `out` and the scratch between guard bands, the scratch exactly the queried size and poisoned beforehand;
    offset: h, out and the scratch that many bytes off the 256-byte grid.  -> (out on the host, status)."""
    _, H, C = h.shape
    width = H * C if concat else C
    nbytes = lib.pope_gat_propagate_scratch_size(n, nnz, H, C, int(concat))
    assert nbytes > 0
    scratch = GuardedScratch(dev, nbytes + offset).fill(fill)
    out = GuardedScratch(dev, n * width * 4 + offset).fill("ones")
    h_buf = torch.empty(n * H * C + 4, dtype=torch.float32, device=dev)
    h_dev = h_buf[offset // 4:offset // 4 + n * H * C]
    h_dev.copy_(torch.from_numpy(h.reshape(-1)))
    at = lambda gs: ctypes.c_void_p(gs.ptr.value + offset)                                              # noqa: E731
    alpha_dev, own_dev = _up(dev, alpha), _up(dev, alpha_self)                      # (named: they live until the call has run)
    rc = lib.pope_gat_propagate(_ptr(csr[0]), _ptr(csr[1]), n, nnz, _ptr(alpha_dev), _ptr(own_dev), _ptr(h_dev), H, C,
                                int(concat), _ptr(bias), at(out), at(scratch), nbytes, _stream())
    torch.cuda.synchronize()
    assert scratch.bands_intact() and out.bands_intact()
    got = out.view[offset:offset + n * width * 4].cpu().numpy().copy().view(np.float32).reshape(n, width)
    return got, rc


@pytest.fixture(scope="module")
def device_alpha(dev, lib, csrs):
    """{(H, C, self_loops): (h, alpha, alpha_self or None, bias)}: the device's own attention of the main graph, computed once."""
    g = cases.graph("main")
    out = {}
    for H, C in HEAD_SHAPES:
        h, att_l, att_r, b = _heads_inputs(H, C)
        for self_loops in (True, False):
            _, _, alpha, alpha_self = _attention(dev, lib, csrs["main", False], g.n, g.nnz, h, att_l, att_r, 0.2, self_loops)
            out[H, C, self_loops] = (h, alpha, alpha_self if self_loops else None, b)
    return out


@pytest.mark.parametrize("concat", (True, False), ids=("concat", "mean"))
@pytest.mark.parametrize("H,C", HEAD_SHAPES)
def test_propagate_bit_for_bit_given_the_device_alpha(H, C, concat, dev, lib, csrs, device_alpha):
    g = cases.graph("main")
    rowptr, col = cases.canonical("main", False)
    for self_loops, has_bias in ((True, True), (False, False), (False, True)):
        h, alpha, alpha_self, b = device_alpha[H, C, self_loops]
        bias = (b if concat else b[:C]) if has_bias else None
        want = cases.propagate_restatement(rowptr, col, g.n, h, alpha, alpha_self, bias, concat)
        got, rc = _propagate(dev, lib, csrs["main", False], g.n, g.nnz, alpha, alpha_self, h, concat, _up(dev, bias))
        assert rc == 0, lib.pope_last_error()
        diff = _bits(got) != _bits(want)
        assert not diff.any(), (self_loops, has_bias, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@pytest.mark.parametrize("H,C", ((4, 64), (2, 130)))
def test_propagate_off_the_16_byte_grid_gives_the_same_bits(H, C, dev, lib, csrs, device_alpha):
    g = cases.graph("main")
    rowptr, col = cases.canonical("main", False)
    h, alpha, alpha_self, b = device_alpha[H, C, True]
    b_buf = torch.zeros(H * C + 1, dtype=torch.float32, device=dev)
    b_buf[1:].copy_(torch.from_numpy(b))
    for concat in (True, False):
        want = cases.propagate_restatement(rowptr, col, g.n, h, alpha, alpha_self, b if concat else b[:C], concat)
        got, rc = _propagate(dev, lib, csrs["main", False], g.n, g.nnz, alpha, alpha_self, h, concat, b_buf[1:], offset=4)
        assert rc == 0, lib.pope_last_error()
        assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("fill", ("zeros", "ones"))
def test_nothing_is_read_before_it_is_written(fill, dev, lib, csrs):
    g = cases.graph("main")
    rowptr, col = cases.canonical("main", False)
    h, att_l, att_r, _ = _heads_inputs(4, 64)
    first = _attention(dev, lib, csrs["main", False], g.n, g.nnz, h, att_l, att_r, 0.2, True, fill="noise")
    again = _attention(dev, lib, csrs["main", False], g.n, g.nnz, h, att_l, att_r, 0.2, True, fill=fill)
    for a, b in zip(first, again):
        assert np.array_equal(_bits(a), _bits(b))
    _, _, alpha, alpha_self = again
    for concat in (True, False):
        want = cases.propagate_restatement(rowptr, col, g.n, h, alpha, alpha_self, None, concat)
        got, rc = _propagate(dev, lib, csrs["main", False], g.n, g.nnz, alpha, alpha_self, h, concat, None, fill=fill)
        assert rc == 0 and np.array_equal(_bits(got), _bits(want))


def test_a_scratch_one_byte_short_is_refused_and_nothing_is_written(dev, lib, csrs, device_alpha):
    from graphpope_amd import _lib
    g = cases.graph("main")
    rowptr, col = csrs["main", False]
    rowptr_t, col_t = csrs["main", True]
    h, alpha, alpha_self, _ = device_alpha[4, 64, True]
    nbytes = lib.pope_gat_propagate_scratch_size(g.n, g.nnz, 4, 64, 0)
    scratch = GuardedScratch(dev, nbytes).fill("noise")
    out = GuardedScratch(dev, g.n * 64 * 4).fill("noise")
    before, before_out = scratch.snapshot(), out.snapshot()
    ptr, short = scratch.short(1)
    alpha_dev, own_dev, h_dev = _up(dev, alpha), _up(dev, alpha_self), _up(dev, h)
    rc = lib.pope_gat_propagate(_ptr(rowptr), _ptr(col), g.n, g.nnz, _ptr(alpha_dev), _ptr(own_dev), _ptr(h_dev), 4, 64, 0,
                                None, out.ptr, ptr, short, _stream())
    assert rc == _lib.ERR_WORKSPACE and str(nbytes).encode() in lib.pope_last_error()
    assert scratch.unchanged_since(before) and out.unchanged_since(before_out)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)                              # noqa: E731
    x, w, att, hh, a, al, ga = z(g.n, 36), z(256, 36), z(4, 64), z(g.n, 256), z(g.n, 4), z(g.nnz, 4), z(2, 4, 64)
    slots = torch.zeros(g.nnz, dtype=torch.int32, device=dev)
    for which in ("forward", "backward"):
        query = lib.pope_gat_conv_forward_scratch_size if which == "forward" else lib.pope_gat_conv_backward_scratch_size
        need = query(g.n, g.nnz, 36, 4, 64, 1)
        s = GuardedScratch(dev, need).fill("noise")
        o = GuardedScratch(dev, g.n * 256 * 4).fill("noise")
        snap, snap_o = s.snapshot(), o.snapshot()
        if which == "forward":
            rc = lib.pope_gat_conv_forward(_ptr(rowptr), _ptr(col), g.n, g.nnz, _ptr(x), 36, _ptr(w), _ptr(att), _ptr(att), None, 4, 64, 1, 0.2, 1,
                                           _ptr(hh), _ptr(a), _ptr(a), _ptr(al), _ptr(a), o.ptr, s.ptr, need - 1, _stream())
        else:
            rc = lib.pope_gat_conv_backward(_ptr(rowptr), _ptr(col), _ptr(rowptr_t), _ptr(col_t), _ptr(slots), g.n, g.nnz, _ptr(x), 36, _ptr(w), _ptr(att), _ptr(att), 4, 64, 1, 0.2, 1, _ptr(hh), _ptr(a), _ptr(a),
                                            _ptr(al), _ptr(a), _ptr(hh), None, o.ptr, _ptr(ga[0]), _ptr(ga[1]), None, s.ptr, need - 1, _stream())
        assert rc == _lib.ERR_WORKSPACE and str(need).encode() in lib.pope_last_error(), which
        assert s.unchanged_since(snap) and o.unchanged_since(snap_o), which


def test_single_with_self_loops_returns_h_plus_b_and_empty_without_returns_b(dev, lib, csrs):
    rs = np.random.RandomState(9)
    for name, self_loops in (("single", True), ("empty", True), ("empty", False), ("single", False)):
        g = cases.graph(name)
        H, C = 2, 130
        h = rs.randn(g.n, H, C).astype(np.float32)
        att_l, att_r, b = rs.randn(H, C).astype(np.float32), rs.randn(H, C).astype(np.float32), rs.randn(H * C).astype(np.float32)
        a_src, a_dst, alpha, alpha_self = _attention(dev, lib, csrs[name, False], g.n, 0, h, att_l, att_r, 0.2, self_loops)
        assert alpha.size == 0 and (alpha_self == (1.0 if self_loops else 0.0)).all()
        got, rc = _propagate(dev, lib, csrs[name, False], g.n, 0, None, alpha_self if self_loops else None, h, True, _up(dev, b))
        want = (h.reshape(g.n, H * C) + b) if self_loops else np.broadcast_to(b, (g.n, H * C))
        assert rc == 0 and np.array_equal(_bits(got), _bits(want)), (name, self_loops)


# ------------------------------------------------------------------------------------------------ the layer against float64

def _device_layer(dev, adj, case):
    """-> (tensors, pattern): out and the gradients, and the device's LeakyReLU pattern from its own float32 scores."""
    from graphpope_amd import gat
    t = cases.layer_inputs(case)
    conv = gat.GATConv(case.c_in, case.C, heads=case.H, concat=case.concat, negative_slope=case.negative_slope,
                       add_self_loops=case.add_self_loops, bias=case.bias).to(dev)
    with torch.no_grad():
        for k in cases.PARAM_KEYS:
            if k != "bias" or case.bias:
                dict(conv.named_parameters())[k].copy_(torch.from_numpy(t[k]))
    x = torch.from_numpy(t["x"]).to(dev).requires_grad_(case.grad_x)
    out, (alpha, alpha_self) = conv(x, adj, return_attention_weights=True)
    saved = out.grad_fn.saved_tensors                                  # x, w, att_l, att_r, h, a_src, a_dst, alpha, alpha_self
    pattern = cases.device_pattern(saved[5], saved[6])
    assert alpha.shape == (adj.nnz, case.H) and alpha_self.shape == (adj.num_nodes, case.H) and not alpha.requires_grad
    (out * torch.from_numpy(t["g"]).to(dev)).sum().backward()
    got = {"out": out.detach().cpu(), "grad_lin_l.weight": conv.lin_l.weight.grad.cpu(), "grad_att_l": conv.att_l.grad.cpu(),
           "grad_att_r": conv.att_r.grad.cpu()}
    if case.grad_x:
        got["grad_x"] = x.grad.cpu()
    if case.bias:
        got["grad_bias"] = conv.bias.grad.cpu()
    return got, pattern


@pytest.mark.parametrize("case", cases.LAYER_CASES, ids=lambda c: c.id)
def test_layer_out_and_every_gradient_within_the_rule(case, dev, adj):
    got, pattern = _device_layer(dev, adj, case)
    t64, err32, gated, mismatches = cases.layer_expectation(case, pattern)
    assert cases.gate_share(case) <= cases.EXCLUDED_CAP and mismatches == 0, (gated, mismatches)
    assert set(got) == set(t64) - (set() if case.grad_x else {"grad_x"})
    report = {k: (cases.err(got[k], t64[k]), cases.threshold(err32[k])) for k in got}
    print(case.id, "gated", gated, {k: "%.3g / %.3g" % v for k, v in report.items()})
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    for k, (e, bound) in report.items():
        assert e <= bound, (k, e, bound)


# ------------------------------------------------------------------------------------------------ the model

def _device_model(dev, dropout=0.0):
    from graphpope_amd import gat
    t = cases.model_inputs()
    model = gat.GAT(cases.MODEL_IN, cases.MODEL_HIDDEN, cases.MODEL_OUT, num_layers=2, heads=cases.MODEL_HEADS, dropout=dropout).to(dev)
    model.load_state_dict({k: torch.from_numpy(t[k]) for k in cases.PARAMS})
    return model, torch.from_numpy(t["x"]).to(dev), torch.from_numpy(t["y"]).to(dev)


def _model_step(model, x, y, adj):
    from graphpope_amd import sage
    patterns = []
    hooks = [c.register_forward_hook(lambda m, i, o: patterns.append(cases.device_pattern(*o.grad_fn.saved_tensors[5:7]))) for c in model.convs]
    for p in model.parameters():
        p.grad = None
    logits = model(x, adj)
    loss = sage.cross_entropy(logits, y)
    loss.backward()
    for hook in hooks:
        hook.remove()
    got = {"logits": logits.detach().cpu(), "loss": float(loss.detach())}
    got.update({"grad:" + k: p.grad.cpu() for k, p in model.named_parameters()})
    return got, patterns


def test_two_layer_model_loss_and_every_gradient(dev, adj):
    model, x, y = _device_model(dev)
    got, patterns = _model_step(model, x, y, adj)
    ref, err32, share, mismatches = cases.model_expectation(patterns)
    assert share <= cases.EXCLUDED_CAP and mismatches == 0, (share, mismatches)
    report = {k: (cases.err(got[k], ref[k]), cases.threshold(err32[k])) for k in err32}
    print({k: "%.3g / %.3g" % v for k, v in report.items()}, "loss", abs(got["loss"] - ref["loss"]), cases.loss_bound(ref, err32))
    for k, (e, bound) in report.items():
        assert e <= bound, (k, e, bound)
    assert abs(got["loss"] - ref["loss"]) <= cases.loss_bound(ref, err32)


def test_forward_and_backward_are_bit_reproducible_in_both_modes(dev, adj):
    from graphpope_amd import sage
    model, x, y = _device_model(dev)
    runs = []
    for mode in (False, False, True, True):
        with sage.deterministic(mode):
            got, _ = _model_step(model, x, y, adj)
        runs.append({k: _bits(v.numpy()) for k, v in got.items() if k != "loss"})
    for other in runs[1:]:
        for k, bits in runs[0].items():
            assert np.array_equal(bits, other[k]), k


def test_training_smoke(dev):
    """A planted-partition graph, 40 full-batch steps at dropout 0.5 through the product's loss and optimiser: the loss falls, every
    parameter stays finite and the model separates the classes."""
    from graphpope_amd import gat, optim, sage
    ei, x, y = cases.planted_partition()
    torch.manual_seed(3)
    adj = gat.GraphAdj(torch.from_numpy(ei).to(dev), x.shape[0])
    model = gat.GAT(16, 32, 3, num_layers=2, heads=4, dropout=0.5).to(dev)
    opt = optim.Adam(model.parameters(), lr=0.02, max_grad_norm=0.5)
    x, y = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    losses = []
    model.train()
    for _ in range(40):
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


def test_command_line_trains_a_gat(tmp_path):
    """GRAPHPOPE_MODEL=gcn GRAPHPOPE_GCN_LAYER=gat python -m graphpope_amd.main --dataset pubmed --epochs 2 --num_layers 2 in a child
    process (the synthetic PubMed-shaped graph): exit 0, two epoch lines and a test_acc line at the end."""
    env = dict(os.environ, GRAPHPOPE_MODEL="gcn", GRAPHPOPE_GCN_LAYER="gat", GRAPHPOPE_DATA_DIR=str(tmp_path))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GRAPHPOPE_GAT_HEADS"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "graphpope_amd.main", "--dataset", "pubmed", "--epochs", "2", "--num_layers", "2"]
    proc = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, errs = proc.communicate(timeout=240.0)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.communicate()
        pytest.fail("GRAPHPOPE_MODEL=gcn GRAPHPOPE_GCN_LAYER=gat python -m graphpope_amd.main did not finish within 240 s")
    assert proc.returncode == 0, errs[-4000:]
    lines = [line for line in out.splitlines() if line.strip()]
    assert [line.split(":")[0] for line in lines if line.startswith("epoch ")] == ["epoch 0", "epoch 1"]
    assert lines[-1].startswith("test_acc ") and 0.0 <= float(lines[-1].split()[1]) <= 1.0
