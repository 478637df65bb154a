"""Cases, float64 reference, float32 restatements and the threshold for GATConv / GAT on the whole graph (include/graphpope_hip.h:
pope_gat_*; graphpope_amd/gat.py).  Imports without a GPU and is not a test module: test_gat_cpu.py proves the reference, the gate and the
restatements on the CPU, test_gat_gpu.py runs the kernels through them.

Graph: full_inference_cases.graph("main") (300 nodes, 4 029 slots, 58 self-loops, repeated edges, degrees 0 .. 1 025: both edges of the
hub path), "single" and "empty".  :func:`canonical` is a CSR with ascending rows, by destination or by source, as GraphAdj builds them;
:func:`slot_map_restatement` the edge correspondence between the two.

Reference (:func:`dense_layer`): float64 under autograd, per head a masked [N, N] softmax.  M[i, j] = how often row i holds j (with self
loops the diagonal is replaced by 1); alpha_ij = exp(e'_ij - m_i) / sum_j M_ij exp(e'_ij - m_i) per copy, agg_i = sum_j M_ij alpha_ij h_j:
repeated edges are separate terms.  It shares no structure with the kernels.
Restatement (:func:`edge_layer`): float32, edge by edge (index_select, scatter_reduce amax, exp, index_add_) under PERMS permutations of
the edge order; for the bias gradient the rows of the upstream gradient are permuted as well.
Documented order: :func:`scores_restatement` and :func:`propagate_restatement`, NumPy float32 operation by operation; the device must
give these bits (the propagate: given the device's own alpha).

Error measure and threshold: gcn_cases.py's.  err(T) = max |T - T_64| / max |T_64|,  err_dev <= FACTOR * max(err_32, 2^-23), FACTOR = 4.

LeakyReLU kink gate: a term is gated when |e_64| < GATE * std(e_64) (std over all terms of the layer), GATE = 2^-12.  Inside the gate the
reference takes the device's pattern (the float32 sum a_src[j] + a_dst[i] > 0 of the device's own scores), outside it the device's pattern
must equal the reference's.  The gated share is at most bn_epilogue_cases.EXCLUDED_CAP.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import bn_epilogue_cases as bn
import full_inference_cases as fic
import gcn_cases

CHUNK = fic.CHUNK
PERMS = 6
FACTOR = 4.0
FLOOR = 2.0 ** -23
GATE = 2.0 ** -12
CUS = 256
EXCLUDED_CAP = bn.EXCLUDED_CAP

graph = fic.graph
err = fic.err
planted_partition = gcn_cases.planted_partition


def threshold(err32: float) -> float:
    return FACTOR * max(err32, FLOOR)


@functools.lru_cache(maxsize=None)
def canonical(name: str = "main", by_source: bool = False):
    """(rowptr, col) int32 with every row ascending (repeated edges adjacent): by destination (row i lists its sources) or by source."""
    g = graph(name)
    rows, ids = (g.src, g.dst) if by_source else (g.dst, g.src)
    order = np.lexsort((ids, rows))
    rowptr = np.zeros(g.n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=g.n))
    return rowptr.astype(np.int32), ids[order].astype(np.int32)


def slot_map_restatement(name: str = "main") -> np.ndarray:
    """int32 [nnz]: for slot q = (j -> i) of the CSR by source the slot of the CSR by destination holding that edge: the first j in row i
    plus q's rank among the equal ids of its own row."""
    g = graph(name)
    rowptr, col = canonical(name, False)
    rowptr_t, col_t = canonical(name, True)
    out = np.full(g.nnz, -1, dtype=np.int32)
    for j in range(g.n):
        for q in range(rowptr_t[j], rowptr_t[j + 1]):
            i = int(col_t[q])
            first = rowptr_t[j] + int(np.searchsorted(col_t[rowptr_t[j]:rowptr_t[j + 1]], i, side="left"))
            pos = rowptr[i] + int(np.searchsorted(col[rowptr[i]:rowptr[i + 1]], j, side="left"))
            out[q] = pos + (q - first)
    return out


# ------------------------------------------------------------------------------------------------ the documented order, bit for bit

def scores_restatement(h, att) -> np.ndarray:
    """[n, H] float32: a = +0, then a = a + h[i, k, c] * att[k, c] for c ascending (h [n, H, C], att [H, C])."""
    f32 = np.float32
    h, att = np.asarray(h, dtype=f32), np.asarray(att, dtype=f32)
    a = np.zeros(h.shape[:2], dtype=f32)
    for c in range(h.shape[2]):
        a = a + (h[:, :, c] * att[None, :, c]).astype(f32)
    return a


def propagate_restatement(rowptr, col, n, h, alpha, alpha_self=None, bias=None, concat=True) -> np.ndarray:
    """out float32 in the order include/graphpope_hip.h documents, alpha [nnz, H] given: h [n, H, C]; alpha_self [n, H] or None (no self
    term, self-loop slots ordinary).  concat: [n, H C]; else the head sum ascending, / (float)H, + bias."""
    f32 = np.float32
    h = np.asarray(h, dtype=f32)
    _, H, C = h.shape
    agg = np.zeros_like(h)
    zero = np.zeros((H, C), dtype=f32)
    skip_self = alpha_self is not None
    for i in range(n):
        beg, end = int(rowptr[i]), int(rowptr[i + 1])

        def run(lo, hi):
            s = zero.copy()
            for p in range(lo, hi):
                j = int(col[p])
                if j < 0 or j >= n or (skip_self and j == i):
                    continue
                s = s + (alpha[p][:, None] * h[j]).astype(f32)
            return s

        if end - beg <= CHUNK:
            s = run(beg, end)
        else:
            s = zero.copy()
            for lo in range(beg, end, CHUNK):                       # runs of CHUNK slot positions, skipped slots included
                s = s + run(lo, min(lo + CHUNK, end))
        if skip_self:
            s = s + (alpha_self[i][:, None] * h[i]).astype(f32)
        agg[i] = s
    if concat:
        out = agg.reshape(n, H * C)
        return out if bias is None else out + np.asarray(bias, dtype=f32)
    o = np.zeros((n, C), dtype=f32)
    for k in range(H):
        o = o + agg[:, k, :]
    o = (o / f32(H)).astype(f32)
    return o if bias is None else o + np.asarray(bias, dtype=f32)


# ------------------------------------------------------------------------------------------------ layer cases

@dataclass(frozen=True)
class LayerCase:
    c_in: int
    H: int
    C: int
    concat: bool = True
    bias: bool = True
    grad_x: bool = True
    add_self_loops: bool = True
    negative_slope: float = 0.2
    att_scale: float = 1.0
    graph: str = "main"

    @property
    def id(self):
        tags = [f"{self.c_in}x{self.H}x{self.C}"] + [t for t, on in (("mean", not self.concat), ("nobias", not self.bias),
                                                                     ("nogradx", not self.grad_x), ("noself", not self.add_self_loops),
                                                                     ("slope0", self.negative_slope == 0.0), ("overflow", self.att_scale != 1.0)) if on]
        return "-".join(tags)

    @property
    def width(self):
        return self.H * self.C if self.concat else self.C


SHAPES = ((36, 1, 64), (36, 4, 64), (36, 8, 8), (12, 3, 7), (36, 2, 130), (37, 1, 5))
OVERFLOW_CASE = LayerCase(36, 4, 64, att_scale=400.0)
LAYER_CASES = tuple(LayerCase(*s) for s in SHAPES) + (
    LayerCase(36, 4, 64, concat=False), LayerCase(36, 4, 64, bias=False), LayerCase(36, 4, 64, grad_x=False),
    LayerCase(36, 4, 64, add_self_loops=False), LayerCase(36, 4, 64, negative_slope=0.0), LayerCase(12, 3, 7, concat=False), OVERFLOW_CASE)
PARAM_KEYS = ("lin_l.weight", "att_l", "att_r", "bias")


@functools.lru_cache(maxsize=None)
def layer_inputs(case: LayerCase):
    """float32 arrays: x, lin_l.weight [H C, c_in], att_l / att_r [1, H, C], bias, and the upstream gradient g (loss = sum(out * g))."""
    g = graph(case.graph)
    rs = np.random.RandomState(5000 + 17 * case.c_in + 101 * case.H + case.C)
    bound = 1.0 / np.sqrt(case.c_in)
    a = case.att_scale / np.sqrt(case.C)
    return {"x": (0.25 + rs.randn(g.n, case.c_in)).astype(np.float32),
            "lin_l.weight": rs.uniform(-bound, bound, size=(case.H * case.C, case.c_in)).astype(np.float32),
            "att_l": (a * rs.randn(1, case.H, case.C)).astype(np.float32),
            "att_r": (a * rs.randn(1, case.H, case.C)).astype(np.float32),
            "bias": rs.uniform(-bound, bound, size=case.width).astype(np.float32),
            "g": rs.randn(g.n, case.width).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def multiplicity(name: str, self_loops: bool) -> torch.Tensor:
    """float64 [n, n]: M[i, j] = how often row i holds j; with self loops the diagonal is replaced by 1."""
    g = graph(name)
    m = torch.zeros((g.n, g.n), dtype=torch.float64)
    if g.nnz:
        m.index_put_((torch.from_numpy(g.dst), torch.from_numpy(g.src)), torch.ones(g.nnz, dtype=torch.float64), accumulate=True)
    if self_loops:
        m.fill_diagonal_(1.0)
    return m


def _finish(agg, bias, concat):
    n, H, C = agg.shape
    out = agg.reshape(n, H * C) if concat else agg.sum(1) / H
    return out if bias is None else out + bias


def dense_layer(name, x, weight, att_l, att_r, bias, H, C, concat, slope, self_loops, pattern=None):
    """-> (out, e [H, n, n] detached, alpha_w [H, n, n] detached: M_ij alpha_ij).  pattern: bool [H, n, n] (e > 0 where None)."""
    m_ = multiplicity(name, self_loops).to(x.dtype)
    n = x.shape[0]
    h = (x @ weight.t()).view(n, H, C)
    a_s, a_d = (h * att_l.view(1, H, C)).sum(-1), (h * att_r.view(1, H, C)).sum(-1)
    e = a_d.t()[:, :, None] + a_s.t()[:, None, :]                                   # [H, i, j]
    pat = (e.detach() > 0) if pattern is None else pattern
    e2 = torch.where(pat, e, slope * e)
    mask = (m_ > 0)[None]
    e2m = e2.masked_fill(~mask, float("-inf"))
    top = e2m.detach().max(dim=2, keepdim=True).values
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    ex = torch.exp(e2m - top) * m_[None]
    s = ex.sum(2, keepdim=True)
    w = ex / torch.where(s > 0, s, torch.ones_like(s))
    agg = torch.einsum("kij,jkc->ikc", w, h)
    return _finish(agg, bias, concat), e.detach(), w.detach()


def _edges(name, self_loops, perm_seed):
    """(src, dst) int64 tensors of the terms: with self loops the self-loop slots dropped and one i -> i per node appended."""
    g = graph(name)
    src, dst = g.src, g.dst
    if self_loops:
        keep = src != dst
        loops = np.arange(g.n, dtype=np.int64)
        src, dst = np.concatenate([src[keep], loops]), np.concatenate([dst[keep], loops])
    if perm_seed is not None and src.size:
        p = np.random.RandomState(900 + perm_seed).permutation(src.size)
        src, dst = src[p], dst[p]
    return torch.from_numpy(src), torch.from_numpy(dst)


def edge_layer(name, x, weight, att_l, att_r, bias, H, C, concat, slope, self_loops, perm_seed, pattern=None):
    """The layer edge by edge in x's dtype, stock torch ops over the (permuted) term list."""
    src, dst = _edges(name, self_loops, perm_seed)
    n = x.shape[0]
    h = (x @ weight.t()).view(n, H, C)
    if src.numel() == 0:
        return _finish(torch.zeros_like(h) * h, bias, concat)
    a_s, a_d = (h * att_l.view(1, H, C)).sum(-1), (h * att_r.view(1, H, C)).sum(-1)
    e = a_s.index_select(0, src) + a_d.index_select(0, dst)                         # [E, H]
    pat = (e.detach() > 0) if pattern is None else pattern[:, dst, src].t()
    e2 = torch.where(pat, e, slope * e)
    idx = dst[:, None].expand(-1, H)
    top = torch.full((n, H), float("-inf"), dtype=x.dtype).scatter_reduce(0, idx, e2.detach(), "amax", include_self=True)
    ex = torch.exp(e2 - top.index_select(0, dst))
    s = torch.zeros((n, H), dtype=x.dtype).index_add_(0, dst, ex)
    alpha = ex / s.index_select(0, dst)
    agg = torch.zeros_like(h).index_add_(0, dst, alpha[:, :, None] * h.index_select(0, src))
    return _finish(agg, bias, concat)


def _layer_tensors(case: LayerCase, forward, dtype):
    """out and the gradients of sum(out * g) as a dict of tensors."""
    t = {k: torch.from_numpy(v).to(dtype) for k, v in layer_inputs(case).items()}
    x = t["x"].requires_grad_(True)
    w, al, ar = (t[k].requires_grad_(True) for k in ("lin_l.weight", "att_l", "att_r"))
    b = t["bias"].requires_grad_(True) if case.bias else None
    out = forward(x, w, al, ar, b)
    (out * t["g"]).sum().backward()
    got = {"out": out.detach(), "grad_x": x.grad, "grad_lin_l.weight": w.grad, "grad_att_l": al.grad, "grad_att_r": ar.grad}
    if case.bias:
        got["grad_bias"] = b.grad
    return got


def _bias_grad_draws(case: LayerCase):
    g = torch.from_numpy(layer_inputs(case)["g"])
    draws = []
    for k in range(PERMS):
        p = torch.from_numpy(np.random.RandomState(1300 + k).permutation(g.shape[0]))
        draws.append(g.index_select(0, p).sum(0))
        acc = torch.zeros(g.shape[1])
        for r in p.tolist():
            acc = acc + g[r]
        draws.append(acc)
    return draws


def _conf(case: LayerCase):
    return case.H, case.C, case.concat, case.negative_slope, case.add_self_loops


@functools.lru_cache(maxsize=None)
def layer_gate(case: LayerCase):
    """(e_64 [H, n, n], terms bool [H, n, n], gated bool [H, n, n]) of the unresolved float64 reference."""
    t = {k: torch.from_numpy(v).double() for k, v in layer_inputs(case).items()}
    _, e, _ = dense_layer(case.graph, t["x"], t["lin_l.weight"], t["att_l"], t["att_r"], None, *_conf(case))
    terms = (multiplicity(case.graph, case.add_self_loops) > 0)[None].expand_as(e)
    if not bool(terms.any()):
        return e, terms, torch.zeros_like(terms)
    gated = terms & (e.abs() < GATE * float(e[terms].std()))
    return e, terms, gated


def gate_share(case: LayerCase) -> float:
    _, terms, gated = layer_gate(case)
    return float(gated.sum()) / max(float(terms.sum()), 1.0)


def device_pattern(a_src, a_dst) -> torch.Tensor:
    """bool [H, n, n] from the device's float32 scores [n, H]: (a_src[j, k] + a_dst[i, k]) > 0, the sum in float32."""
    a_src, a_dst = a_src.float().cpu(), a_dst.float().cpu()
    return (a_dst.t()[:, :, None] + a_src.t()[:, None, :]) > 0


def resolve_pattern(case: LayerCase, device_on=None):
    """(pattern, gated count, mismatches): the reference's pattern with the device's inside the gate; mismatches: terms outside the gate
    where the device's pattern differs."""
    e, terms, gated = layer_gate(case)
    pattern, mismatches = e > 0, None
    if device_on is not None:
        mismatches = int(((device_on != pattern) & terms & ~gated).sum())
        pattern = torch.where(gated, device_on, pattern)
    return pattern, int(gated.sum()), mismatches


_EXPECT = {}


def layer_expectation(case: LayerCase, device_on=None):
    """(T_64, err_32, gated, mismatches): the reference under the resolved pattern and, per tensor, the largest error of the float32
    restatements under the same pattern.  Computed once per (case, pattern inside the gate)."""
    pattern, n_gated, mismatches = resolve_pattern(case, device_on)
    _, _, gated = layer_gate(case)
    key = (case, tuple(pattern[gated].tolist()))
    if key not in _EXPECT:
        conf = _conf(case)
        t64 = _layer_tensors(case, lambda x, w, al, ar, b: dense_layer(case.graph, x, w, al, ar, b, *conf, pattern=pattern)[0], torch.float64)
        err32 = {k: 0.0 for k in t64}
        for perm in (None, *range(PERMS)):
            got = _layer_tensors(case, lambda x, w, al, ar, b: edge_layer(case.graph, x, w, al, ar, b, *conf, perm, pattern=pattern), torch.float32)
            for k in t64:
                err32[k] = max(err32[k], err(got[k], t64[k]))
        if case.bias:
            err32["grad_bias"] = max([err32["grad_bias"]] + [err(d, t64["grad_bias"]) for d in _bias_grad_draws(case)])
        _EXPECT[key] = (t64, err32)
    return (*_EXPECT[key], n_gated, mismatches)


def reference_alpha(case: LayerCase):
    """(alpha [nnz, H], alpha_self [n, H]) float64 of the unresolved reference, in the slot order of canonical(by destination)."""
    t = {k: torch.from_numpy(v).double() for k, v in layer_inputs(case).items()}
    _, _, w = dense_layer(case.graph, t["x"], t["lin_l.weight"], t["att_l"], t["att_r"], None, *_conf(case))
    m_ = multiplicity(case.graph, case.add_self_loops)
    per_copy = w / torch.where(m_ > 0, m_, torch.ones_like(m_))[None]
    g = graph(case.graph)
    rowptr, col = canonical(case.graph, False)
    rows = torch.from_numpy(np.repeat(np.arange(g.n), np.diff(rowptr)).astype(np.int64))
    cols = torch.from_numpy(col.astype(np.int64))
    alpha = per_copy[:, rows, cols].t().clone()
    if case.add_self_loops:
        alpha[rows == cols] = 0.0
        alpha_self = torch.diagonal(per_copy, dim1=1, dim2=2).t().clone()
    else:
        alpha_self = torch.zeros((g.n, case.H), dtype=torch.float64)
    return alpha, alpha_self


# ------------------------------------------------------------------------------------------------ the two-layer model

MODEL_IN, MODEL_HIDDEN, MODEL_OUT, MODEL_HEADS = 36, 64, 5, 8
MODEL_LAYERS = ((MODEL_IN, MODEL_HEADS, MODEL_HIDDEN // MODEL_HEADS), (MODEL_HIDDEN, 1, MODEL_OUT))
PARAMS = tuple(f"convs.{i}.{k}" for i in range(2) for k in PARAM_KEYS)


@functools.lru_cache(maxsize=None)
def model_inputs():
    g = graph("main")
    rs = np.random.RandomState(78)
    t = {"x": (0.25 + rs.randn(g.n, MODEL_IN)).astype(np.float32), "y": rs.randint(0, MODEL_OUT, size=g.n).astype(np.int64)}
    for i, (ci, H, C) in enumerate(MODEL_LAYERS):
        bound = 1.0 / np.sqrt(ci)
        t[f"convs.{i}.lin_l.weight"] = rs.uniform(-bound, bound, size=(H * C, ci)).astype(np.float32)
        t[f"convs.{i}.att_l"] = (rs.randn(1, H, C) / np.sqrt(C)).astype(np.float32)
        t[f"convs.{i}.att_r"] = (rs.randn(1, H, C) / np.sqrt(C)).astype(np.float32)
        t[f"convs.{i}.bias"] = rs.uniform(-bound, bound, size=H * C).astype(np.float32)
    return t


def model_run(dtype, patterns=(None, None), perm="dense"):
    """GAT(36, 64, 5, heads=8) at dropout 0 + F.cross_entropy over all rows.  perm "dense": the dense formula; else the edge form under that
    permutation.  patterns: per layer the LeakyReLU pattern bool [H, n, n] or None.  -> dict: e0, e1 (scores, dense only), logits, loss,
    grad:<param>."""
    t = model_inputs()
    p = {k: torch.from_numpy(t[k]).to(dtype).requires_grad_(True) for k in PARAMS}
    h, y = torch.from_numpy(t["x"]).to(dtype), torch.from_numpy(t["y"])
    out = {}
    for i, (_, H, C) in enumerate(MODEL_LAYERS):
        args = ("main", h, *(p[f"convs.{i}.{k}"] for k in PARAM_KEYS), H, C, True, 0.2, True)
        if perm == "dense":
            h, out[f"e{i}"], _ = dense_layer(*args, pattern=patterns[i])
        else:
            h = edge_layer(*args, perm, pattern=patterns[i])
        if i == 0:
            h = F.elu(h)
    loss = F.cross_entropy(h, y)
    loss.backward()
    out.update({"logits": h.detach(), "loss": float(loss.detach())})
    out.update({"grad:" + k: v.grad for k, v in p.items()})
    return out


@functools.lru_cache(maxsize=None)
def model_gate():
    """Per layer (e_64, terms, gated) of the unresolved float64 model."""
    ref = model_run(torch.float64)
    terms = multiplicity("main", True) > 0
    gates = []
    for i in range(2):
        e = ref[f"e{i}"]
        tm = terms[None].expand_as(e)
        gates.append((e, tm, tm & (e.abs() < GATE * float(e[tm].std()))))
    return gates


def model_expectation(device_on=None):
    """(ref, err_32, gated share, mismatches): the float64 model under the resolved patterns (the device's inside the gates), the
    restatements' errors under the same patterns."""
    patterns, n_gated, n_terms, mismatches = [], 0, 0, None if device_on is None else 0
    for i, (e, terms, gated) in enumerate(model_gate()):
        pat = e > 0
        if device_on is not None:
            mismatches += int(((device_on[i] != pat) & terms & ~gated).sum())
            pat = torch.where(gated, device_on[i], pat)
        patterns.append(pat)
        n_gated += int(gated.sum())
        n_terms += int(terms.sum())
    ref = model_run(torch.float64, patterns)
    err32 = {k: 0.0 for k in ref if k == "logits" or k.startswith("grad:")}
    for perm in (None, *range(PERMS)):
        got = model_run(torch.float32, patterns, perm)
        for k in err32:
            err32[k] = max(err32[k], err(got[k], ref[k]))
    return ref, err32, n_gated / n_terms, mismatches


def loss_bound(ref, err32) -> float:
    """gcn_cases.py's rule: 2 * (allowed absolute logits error) + 8 * 2^-24 * max |logits_64|."""
    top = float(ref["logits"].abs().max())
    return 2.0 * threshold(err32["logits"]) * top + 8.0 * 2.0 ** -24 * top
