"""GATv2Conv / GATv2 on the GPU, through tests/gatv2_cases.py: e and e_self bit for bit against the NumPy restatement of the header's
order (every head shape, both self-loop settings, slope 0, off the 16-byte grid, the degenerate graphs); alpha within the rule; the
propagate over hl, given the device's own alpha, bit for bit; the layer and the two-layer model, out, loss and every gradient, against
the float64 dense formula within the rule under the per-element LeakyReLU gate; bit-reproducibility in both modes of the library;
nothing read before it is written; the refused short scratch; a training smoke test and the command line."""
import ctypes
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import gatv2_cases as cases
from conftest import ROOT
from workspace import GuardedScratch, dev, lib  # noqa: F401  (the fixtures live in the helper module)

pytestmark = pytest.mark.gpu

HEAD_SHAPES = tuple(s[1:] for s in cases.SHAPES)


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


def _off(dev, a, offset):
    """A device copy of `a` that starts `offset` bytes (a multiple of 4) behind a 256-byte boundary."""
    flat = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    buf = torch.empty(flat.size + 64, dtype=torch.float32, device=dev)
    view = buf[offset // 4:offset // 4 + flat.size]
    view.copy_(torch.from_numpy(flat))
    return view


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _f32(gs, shape):
    return gs.view.cpu().numpy().copy().view(np.float32).reshape(shape)


@pytest.fixture(scope="module")
def csrs(dev):
    """Device copies of the canonical CSRs of every graph: {(name, by_source): (rowptr, col)}."""
    return {(name, t): tuple(_up(dev, a) for a in cases.canonical(name, t)) for name in ("main", "single", "empty") for t in (False, True)}


@pytest.fixture(scope="module")
def adj(dev):
    from graphpope_amd import gcn
    g = cases.graph("main")
    return gcn.GraphAdj(torch.from_numpy(np.stack([g.src, g.dst])).to(dev), g.n)


# ------------------------------------------------------------------------------------------------ e, bit for bit; alpha within the rule

def _heads_inputs(H, C, n, scale=1.0):
    rs = np.random.RandomState(8300 + 31 * H + C)
    return ((0.25 + rs.randn(n, H, C)).astype(np.float32), rs.randn(n, H, C).astype(np.float32),
            (scale * rs.randn(H, C) / np.sqrt(C)).astype(np.float32), rs.randn(H * C).astype(np.float32))


def _attention(dev, lib, csr, n, nnz, hl, hr, att, slope, self_loops, fill="ones", offset=0, scores_only=False):
    """pope_gatv2_attention (or pope_gatv2_scores) with every output between guard bands and pre-filled -> (e, e_self, alpha,
    alpha_self) on the host.  offset: hl, hr and att that many bytes off the 256-byte grid."""
    H, C = hl.shape[1:]
    bufs = [GuardedScratch(dev, size * 4).fill(fill) for size in (nnz * H, n * H, nnz * H, n * H)]
    l_dev, r_dev, a_dev = _off(dev, hl, offset), _off(dev, hr, offset), _off(dev, att, offset)    # (named: they live until the call has run)
    if scores_only:
        rc = lib.pope_gatv2_scores(_ptr(csr[0]), _ptr(csr[1]), n, nnz, _ptr(l_dev), _ptr(r_dev), H, C, _ptr(a_dev), slope, int(self_loops),
                                   bufs[0].ptr, bufs[1].ptr, _stream())
    else:
        rc = lib.pope_gatv2_attention(_ptr(csr[0]), _ptr(csr[1]), n, nnz, _ptr(l_dev), _ptr(r_dev), H, C, _ptr(a_dev), slope, int(self_loops),
                                      *(b.ptr for b in bufs), _stream())
    assert rc == 0, lib.pope_last_error()
    torch.cuda.synchronize()
    assert all(b.bands_intact() for b in bufs)
    return tuple(_f32(b, s) for b, s in zip(bufs, ((nnz, H), (n, H), (nnz, H), (n, H))))


def _e_expected(name, hl, hr, att, slope, self_loops):
    g = cases.graph(name)
    rowptr, col = cases.canonical(name, False)
    rows = np.repeat(np.arange(g.n), np.diff(rowptr))
    e = cases.e_restatement(hl, hr, att, col.astype(np.int64), rows, slope) if g.nnz else np.zeros((0, hl.shape[1]), dtype=np.float32)
    own = np.arange(g.n)
    e_self = cases.e_restatement(hl, hr, att, own, own, slope)
    if self_loops:
        e[col == rows] = 0.0
    else:
        e_self[:] = 0.0
    return e, e_self


def _alpha_from_e(dtype, rowptr, col, n, e, e_self, self_loops):
    """The attention of every slot and of the self term from given scores, row by row in `dtype` (max, exp, sum, divide)."""
    e, e_self = e.astype(dtype), e_self.astype(dtype)
    alpha, own = np.zeros_like(e), np.zeros_like(e_self)
    for i in range(n):
        ids = col[rowptr[i]:rowptr[i + 1]]
        term = (ids != i) if self_loops else np.ones(ids.size, dtype=bool)
        block = e[rowptr[i]:rowptr[i + 1]][term]
        block = np.concatenate([block, e_self[i][None]]) if self_loops else block
        if block.shape[0] == 0:
            continue
        ex = np.exp(block - block.max(0, keepdims=True))
        w = (ex / ex.sum(0, keepdims=True)).astype(dtype)
        out = alpha[rowptr[i]:rowptr[i + 1]]
        out[term] = w[:int(term.sum())]
        if self_loops:
            own[i] = w[-1]
    return alpha, own


@pytest.mark.parametrize("H,C", HEAD_SHAPES)
def test_e_bit_for_bit_on_and_off_the_16_byte_grid_and_alpha_within_the_rule(H, C, dev, lib, csrs):
    g = cases.graph("main")
    rowptr, col = cases.canonical("main", False)
    rows = np.repeat(np.arange(g.n), np.diff(rowptr))
    hl, hr, att, _ = _heads_inputs(H, C, g.n)
    for self_loops, slope, offset in ((True, 0.2, 0), (False, 0.2, 0), (True, 0.0, 0), (True, 0.2, 4), (False, 0.2, 8)):
        e, e_self, alpha, alpha_self = _attention(dev, lib, csrs["main", False], g.n, g.nnz, hl, hr, att, slope, self_loops, offset=offset)
        want, want_self = _e_expected("main", hl, hr, att, slope, self_loops)
        diff = _bits(e) != _bits(want)
        assert not diff.any(), (self_loops, slope, offset, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert np.array_equal(_bits(e_self), _bits(want_self)), (self_loops, slope, offset)
        # the reference and the float32 draw both start from the device's scores: what is tested is the softmax
        ref, ref_self = _alpha_from_e(np.float64, rowptr, col, g.n, e, e_self, self_loops)
        draw, draw_self = _alpha_from_e(np.float32, rowptr, col, g.n, e, e_self, self_loops)
        bound = cases.threshold(max(cases.err(draw, ref), cases.err(draw_self, ref_self) if self_loops else 0.0))
        print((H, C, self_loops, slope, offset), cases.err(alpha, ref), bound)
        assert cases.err(alpha, ref) <= bound and np.isfinite(alpha).all()
        if self_loops:
            assert cases.err(alpha_self, ref_self) <= bound and (alpha[col == rows] == 0).all()
        else:
            assert (alpha_self == 0).all()
        total = np.zeros((g.n, H), dtype=np.float64)
        np.add.at(total, rows, alpha.astype(np.float64))
        total += alpha_self
        has_terms = np.ones(g.n, dtype=bool) if self_loops else np.diff(rowptr) > 0
        assert np.abs(total[has_terms] - 1).max() <= 4 * 2.0 ** -23 and (total[~has_terms] == 0).all()
    only = _attention(dev, lib, csrs["main", False], g.n, g.nnz, hl, hr, att, 0.2, True, fill="zeros", scores_only=True)
    want, want_self = _e_expected("main", hl, hr, att, 0.2, True)
    assert np.array_equal(_bits(only[0]), _bits(want)) and np.array_equal(_bits(only[1]), _bits(want_self))
    same = _attention(dev, lib, csrs["main", False], g.n, g.nnz, hl, hl, att, 0.2, True)                # hr is hl: shared weights
    want, want_self = _e_expected("main", hl, hl, att, 0.2, True)
    assert np.array_equal(_bits(same[0]), _bits(want)) and np.array_equal(_bits(same[1]), _bits(want_self))


@pytest.mark.parametrize("H,C", ((4, 64), (3, 7), (3, 100)))
def test_propagate_over_hl_bit_for_bit_given_the_device_alpha(H, C, dev, lib, csrs):
    g = cases.graph("main")
    rowptr, col = cases.canonical("main", False)
    hl, hr, att, b = _heads_inputs(H, C, g.n)
    for self_loops, concat in ((True, True), (False, True), (True, False)):
        _, _, alpha, alpha_self = _attention(dev, lib, csrs["main", False], g.n, g.nnz, hl, hr, att, 0.2, self_loops)
        own = alpha_self if self_loops else None
        bias = b if concat else b[:C]
        want = cases.propagate_restatement(rowptr, col, g.n, hl, alpha, own, bias, concat)
        width = H * C if concat else C
        nbytes = lib.pope_gat_propagate_scratch_size(g.n, g.nnz, H, C, int(concat))
        scratch, out = GuardedScratch(dev, nbytes).fill("noise"), GuardedScratch(dev, g.n * width * 4).fill("ones")
        h_dev, a_dev, o_dev, b_dev = _up(dev, hl), _up(dev, alpha), _up(dev, own), _up(dev, bias)
        rc = lib.pope_gat_propagate(_ptr(csrs["main", False][0]), _ptr(csrs["main", False][1]), g.n, g.nnz, _ptr(a_dev), _ptr(o_dev), _ptr(h_dev),
                                    H, C, int(concat), _ptr(b_dev), out.ptr, scratch.ptr, nbytes, _stream())
        assert rc == 0, lib.pope_last_error()
        torch.cuda.synchronize()
        assert scratch.bands_intact() and out.bands_intact()
        assert np.array_equal(_bits(_f32(out, (g.n, width))), _bits(want)), (self_loops, concat)


def test_single_and_empty_closed_forms(dev, lib, csrs):
    """No edges: with self loops every alpha_self is 1 and e_self the restatement's; without, everything is 0."""
    for name, self_loops in (("single", True), ("empty", True), ("empty", False), ("single", False)):
        g = cases.graph(name)
        hl, hr, att, _ = _heads_inputs(2, 130, g.n)
        e, e_self, alpha, alpha_self = _attention(dev, lib, csrs[name, False], g.n, 0, hl, hr, att, 0.2, self_loops)
        _, want_self = _e_expected(name, hl, hr, att, 0.2, self_loops)
        assert e.size == 0 and alpha.size == 0 and np.array_equal(_bits(e_self), _bits(want_self))
        assert (alpha_self == (1.0 if self_loops else 0.0)).all()


# ------------------------------------------------------------------------------------------------ the entry points of the layer

def _conv_abi(dev, lib, csrs, case, fill, short=None):
    """pope_gatv2_conv_forward and _backward on the case's inputs with every output and both scratch buffers between guard bands and
    pre-filled.  short: "forward" / "backward" = that call with a scratch one byte short.  -> (dict of host arrays, rc forward, rc
    backward, the guarded buffers)."""
    g = cases.graph(case.graph)
    t = cases.layer_inputs(case)
    H, C, HC, n, nnz, c_in = case.H, case.C, case.H * case.C, g.n, g.nnz, case.c_in
    (rowptr, col), (rowptr_t, col_t) = csrs[case.graph, False], csrs[case.graph, True]
    share = case.share_weights
    d = {k: _up(dev, v) for k, v in t.items()}
    names = {"hl": n * HC, "hr": n * HC, "alpha": nnz * H, "alpha_self": n * H, "out": n * case.width, "grad_x": n * c_in, "grad_wl": HC * c_in,
             "grad_bl": HC, "grad_wr": HC * c_in, "grad_br": HC, "grad_att": HC, "grad_bias": case.width}
    out = {k: GuardedScratch(dev, size * 4).fill(fill) for k, size in names.items()}
    need_f = lib.pope_gatv2_conv_forward_scratch_size(n, nnz, c_in, H, C, int(case.concat))
    need_b = lib.pope_gatv2_conv_backward_scratch_size(n, nnz, c_in, H, C, int(case.concat))
    assert need_f > 0 and need_b > 0
    out["scratch_f"], out["scratch_b"] = GuardedScratch(dev, need_f).fill(fill), GuardedScratch(dev, need_b).fill(fill)
    snaps = {k: b.snapshot() for k, b in out.items()} if short else None
    wr, br = (None, None) if share else (d["lin_r.weight"], d["lin_r.bias"])
    rc_f = lib.pope_gatv2_conv_forward(_ptr(rowptr), _ptr(col), n, nnz, _ptr(d["x"]), c_in, _ptr(d["lin_l.weight"]), _ptr(d["lin_l.bias"]), _ptr(wr),
                                       _ptr(br), _ptr(d["att"]), _ptr(d["bias"]), H, C, int(case.concat), case.negative_slope,
                                       int(case.add_self_loops), out["hl"].ptr, None if share else out["hr"].ptr, out["alpha"].ptr,
                                       out["alpha_self"].ptr, out["out"].ptr, out["scratch_f"].ptr, need_f - (short == "forward"), _stream())
    slot_map = torch.zeros(max(nnz, 1), dtype=torch.int32, device=dev)
    if nnz:
        assert lib.pope_gat_slot_map(_ptr(rowptr), _ptr(col), _ptr(rowptr_t), _ptr(col_t), n, nnz, _ptr(slot_map), _stream()) == 0
    rc_b = lib.pope_gatv2_conv_backward(_ptr(rowptr), _ptr(col), _ptr(rowptr_t), _ptr(col_t), _ptr(slot_map), n, nnz, _ptr(d["x"]), c_in,
                                        _ptr(d["lin_l.weight"]), _ptr(wr), _ptr(d["att"]), H, C, int(case.concat), case.negative_slope,
                                        int(case.add_self_loops), out["hl"].ptr, None if share else out["hr"].ptr, out["alpha"].ptr,
                                        out["alpha_self"].ptr, _ptr(d["g"]), out["grad_x"].ptr, out["grad_wl"].ptr, out["grad_bl"].ptr,
                                        None if share else out["grad_wr"].ptr, None if share else out["grad_br"].ptr, out["grad_att"].ptr,
                                        out["grad_bias"].ptr, out["scratch_b"].ptr, need_b - (short == "backward"), _stream())
    torch.cuda.synchronize()
    assert all(b.bands_intact() for b in out.values())
    skip = {"scratch_f", "scratch_b"} | ({"hr", "grad_wr", "grad_br"} if share else set())
    host = {k: b.view.cpu().numpy().copy() for k, b in out.items() if k not in skip}
    return host, rc_f, rc_b, out, snaps


@pytest.mark.parametrize("case", (cases.LAYER_CASES[1], cases.SHARED_CASE, cases.LAYER_CASES[3], cases.LAYER_CASES[9]), ids=lambda c: c.id)
def test_nothing_is_read_before_it_is_written(case, dev, lib, csrs):
    """Outputs and scratch pre-filled with zeros, then with ones: the same bytes everywhere."""
    first, rc_f, rc_b, _, _ = _conv_abi(dev, lib, csrs, case, "zeros")
    assert rc_f == 0 and rc_b == 0, lib.pope_last_error()
    again, rc_f, rc_b, _, _ = _conv_abi(dev, lib, csrs, case, "ones")
    assert rc_f == 0 and rc_b == 0, lib.pope_last_error()
    for k in first:
        assert np.array_equal(first[k], again[k]), k
        assert np.isfinite(first[k].view(np.float32)).all(), k


def test_a_scratch_one_byte_short_is_refused_and_nothing_is_written(dev, lib, csrs):
    from graphpope_amd import _lib
    case = cases.LAYER_CASES[1]
    _, rc_f, rc_b, bufs, snaps = _conv_abi(dev, lib, csrs, case, "noise", short="forward")
    assert rc_f == _lib.ERR_WORKSPACE and rc_b == 0
    for k in ("hl", "hr", "alpha", "alpha_self", "out", "scratch_f"):
        assert bufs[k].unchanged_since(snaps[k]), k
    _, rc_f, rc_b, bufs, snaps = _conv_abi(dev, lib, csrs, case, "noise", short="backward")
    need = lib.pope_gatv2_conv_backward_scratch_size(300, 4029, 36, 4, 64, 1)
    assert rc_f == 0 and rc_b == _lib.ERR_WORKSPACE and str(need).encode() in lib.pope_last_error()
    for k in ("grad_x", "grad_wl", "grad_bl", "grad_wr", "grad_br", "grad_att", "grad_bias", "scratch_b"):
        assert bufs[k].unchanged_since(snaps[k]), k


def test_no_edges_gives_hl_plus_bias_with_self_loops_and_bias_alone_without(dev, lib, csrs):
    for name in ("single", "empty"):
        for self_loops in (True, False):
            case = cases.LayerCase(12, 2, 130, add_self_loops=self_loops, graph=name)
            host, rc_f, rc_b, _, _ = _conv_abi(dev, lib, csrs, case, "ones")
            assert rc_f == 0 and rc_b == 0, lib.pope_last_error()
            n = cases.graph(name).n
            t = cases.layer_inputs(case)
            got, hl = host["out"].view(np.float32).reshape(n, 260), host["hl"].view(np.float32).reshape(n, 260)
            want = (hl + t["bias"]) if self_loops else np.broadcast_to(t["bias"], (n, 260))
            assert np.array_equal(got, want.astype(np.float32)), (name, self_loops)
            assert cases.err(host["grad_bias"].view(np.float32), t["g"].astype(np.float64).sum(0)) <= 8 * cases.FLOOR
            if not self_loops:                                          # no term at all: only the bias has a gradient
                for k in ("grad_x", "grad_wl", "grad_bl", "grad_wr", "grad_br", "grad_att"):
                    assert not host[k].view(np.float32).any(), (name, k)


# ------------------------------------------------------------------------------------------------ the layer against float64

def _device_layer(dev, adj, case):
    """-> (tensors, pattern, alpha, alpha_self): out and the gradients, and the device's LeakyReLU pattern from its own float32 hl, hr."""
    from graphpope_amd import gatv2
    t = cases.layer_inputs(case)
    conv = gatv2.GATv2Conv(case.c_in, case.C, heads=case.H, concat=case.concat, negative_slope=case.negative_slope,
                           add_self_loops=case.add_self_loops, bias=case.bias, share_weights=case.share_weights).to(dev)
    params = dict(conv.named_parameters())
    assert sorted(params) == sorted(case.param_keys)
    with torch.no_grad():
        for k in case.param_keys:
            params[k].copy_(torch.from_numpy(t[k]))
    x = torch.from_numpy(t["x"]).to(dev).requires_grad_(case.grad_x)
    out, (alpha, alpha_self) = conv(x, adj, return_attention_weights=True)
    saved = out.grad_fn.saved_tensors                                  # x, w_l, w_r, att, hl, hr, alpha, alpha_self
    pattern = cases.device_pattern(saved[4], saved[5], case.H, case.C)
    assert alpha.shape == (adj.nnz, case.H) and alpha_self.shape == (adj.num_nodes, case.H) and not alpha.requires_grad
    (out * torch.from_numpy(t["g"]).to(dev)).sum().backward()
    got = {"out": out.detach().cpu()}
    got.update({"grad_" + k: params[k].grad.cpu() for k in case.param_keys})
    if case.grad_x:
        got["grad_x"] = x.grad.cpu()
    return got, pattern, alpha.cpu(), alpha_self.cpu()


@pytest.mark.parametrize("case", cases.LAYER_CASES, ids=lambda c: c.id)
def test_layer_out_and_every_gradient_within_the_rule(case, dev, adj):
    got, pattern, alpha, alpha_self = _device_layer(dev, adj, case)
    t64, err32, gated, mismatches = cases.layer_expectation(case, pattern)
    assert cases.gate_share(case) <= cases.EXCLUDED_CAP and mismatches == 0, (gated, mismatches)
    assert set(got) == set(t64) - (set() if case.grad_x else {"grad_x"})
    report = {k: (cases.err(got[k], t64[k]), cases.threshold(err32[k])) for k in got}
    print(case.id, "gated", gated, {k: "%.3g / %.3g" % v for k, v in report.items()})
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    for k, (e, bound) in report.items():
        assert e <= bound, (k, e, bound)
    ref, ref_self, err32_alpha = cases.alpha_expectation(case, pattern)
    bound = cases.threshold(err32_alpha)
    print(case.id, "alpha %.3g alpha_self %.3g / %.3g" % (cases.err(alpha, ref), cases.err(alpha_self, ref_self) if case.add_self_loops else 0.0, bound))
    assert bool(torch.isfinite(alpha).all()) and cases.err(alpha, ref) <= bound
    assert cases.err(alpha_self, ref_self) <= bound if case.add_self_loops else not bool(alpha_self.any())


# ------------------------------------------------------------------------------------------------ the model

def _device_model(dev, dropout=0.0):
    from graphpope_amd import gatv2
    t = cases.model_inputs()
    model = gatv2.GATv2(cases.MODEL_IN, cases.MODEL_HIDDEN, cases.MODEL_OUT, num_layers=2, heads=cases.MODEL_HEADS, dropout=dropout).to(dev)
    model.load_state_dict({k: torch.from_numpy(t[k]) for k in cases.PARAMS})
    return model, torch.from_numpy(t["x"]).to(dev), torch.from_numpy(t["y"]).to(dev)


def _model_step(model, x, y, adj):
    from graphpope_amd import sage
    patterns = []
    hooks = [c.register_forward_hook(lambda m, i, o: patterns.append(cases.device_pattern(*o.grad_fn.saved_tensors[4:6], m.heads, m.out_channels)))
             for c in model.convs]
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
    from graphpope_amd import gatv2, optim, sage
    ei, x, y = cases.planted_partition()
    torch.manual_seed(3)
    adj = gatv2.GraphAdj(torch.from_numpy(ei).to(dev), x.shape[0])
    model = gatv2.GATv2(16, 32, 3, num_layers=2, heads=4, dropout=0.5).to(dev)
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


def test_command_line_trains_a_gatv2(tmp_path):
    """GRAPHPOPE_MODEL=gcn GRAPHPOPE_GCN_LAYER=gatv2 python -m graphpope_amd.main --dataset pubmed --epochs 2 --num_layers 2 in a child
    process (the synthetic PubMed-shaped graph): exit 0, two epoch lines and a test_acc line at the end."""
    env = dict(os.environ, GRAPHPOPE_MODEL="gcn", GRAPHPOPE_GCN_LAYER="gatv2", GRAPHPOPE_DATA_DIR=str(tmp_path))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GRAPHPOPE_GAT_HEADS"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "graphpope_amd.main", "--dataset", "pubmed", "--epochs", "2", "--num_layers", "2"]
    proc = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, errs = proc.communicate(timeout=240.0)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.communicate()
        pytest.fail("GRAPHPOPE_MODEL=gcn GRAPHPOPE_GCN_LAYER=gatv2 python -m graphpope_amd.main did not finish within 240 s")
    assert proc.returncode == 0, errs[-4000:]
    lines = [line for line in out.splitlines() if line.strip()]
    assert [line.split(":")[0] for line in lines if line.startswith("epoch ")] == ["epoch 0", "epoch 1"]
    assert lines[-1].startswith("test_acc ") and 0.0 <= float(lines[-1].split()[1]) <= 1.0
