"""Cases, float64 reference, float32 restatements and the threshold for GATv2Conv / GATv2 on the whole graph (include/graphpope_hip.h:
pope_gatv2_*; graphpope_amd/gatv2.py).  Imports without a GPU and is not a test module: test_gatv2_cpu.py proves the reference, the gate
and the restatements on the CPU, test_gatv2_gpu.py runs the kernels through them.  Graphs, canonical CSRs, the propagate's restatement,
the error measure and the threshold are gat_cases.py's (which takes them from gcn_cases.py): err(T) = max |T - T_64| / max |T_64|,
err_dev <= FACTOR * max(err_32, 2^-23), FACTOR = 4.

Reference (:func:`dense_layer`): float64 under autograd, per head and per block of destination rows a masked [B, N] softmax over
z[i, j, :] = hl[j] + hr[i] with multiplicities (gat_cases.multiplicity), so that no more than a few hundred MB live at once.  It shares no
structure with the kernels.
Restatement (:func:`edge_layer`): float32, edge by edge in stock torch ops (index_select twice, the [E, H, C] leaky, the att reduction,
scatter_reduce amax, exp, index_add_) under PERMS permutations of the term list; for the bias gradient the rows of the upstream gradient
are permuted as in gat_cases.
Documented order of e: :func:`e_restatement`, NumPy float32 operation by operation, lane by lane; the device must give these bits.

LeakyReLU kink gate, per element of z: gated when |z_64| < GATE * std(z_64) (std over all terms' elements of the layer), GATE = 2^-12.
Inside the gate the reference takes the device's pattern (hl[j] + hr[i] > 0, summed in float32 from the hl and hr the forward call
returned), outside it the device's pattern must equal the reference's.  The gated share is at most bn_epilogue_cases.EXCLUDED_CAP.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import gat_cases as gc

CHUNK, PERMS, FACTOR, FLOOR, GATE, CUS, EXCLUDED_CAP = gc.CHUNK, gc.PERMS, gc.FACTOR, gc.FLOOR, gc.GATE, gc.CUS, gc.EXCLUDED_CAP
graph, err, threshold, canonical, planted_partition = gc.graph, gc.err, gc.threshold, gc.canonical, gc.planted_partition
propagate_restatement, multiplicity, loss_bound = gc.propagate_restatement, gc.multiplicity, gc.loss_bound
ROW_BLOCK = 64


# ------------------------------------------------------------------------------------------------ the documented order of e, bit for bit

def fold_restatement(t, H, C) -> np.ndarray:
    """[T, H] float32 from the terms t [T, H C] float32 in the order include/graphpope_hip.h documents: slabs of 256 columns, lane l holds
    the columns c0 + 4 l + q, the segmented fold d = 1, 2, .. 32 over the lanes of a head, the head's first lane, slabs ascending."""
    f32 = np.float32
    t = np.asarray(t, dtype=f32)
    T, HC = t.shape
    assert HC == H * C
    e = np.zeros((T, H), dtype=f32)
    lanes = np.arange(64)
    for c0 in range(0, HC, 256):
        c_end = min(HC, c0 + 256)
        slab = np.zeros((T, 256), dtype=f32)
        slab[:, :c_end - c0] = t[:, c0:c_end]
        q = slab.reshape(T, 64, 4)
        cols = c0 + np.arange(256).reshape(64, 4)
        head = np.where(cols < HC, cols // C, -1)
        if C % 4 == 0:
            u = ((q[:, :, 0] + q[:, :, 1]) + q[:, :, 2]) + q[:, :, 3]
            planes = [(u, head[:, 0])]
        else:
            planes = [(q[:, :, k].copy(), head[:, k]) for k in range(4)]
        folded = []
        for u, hd in planes:
            for d in (1, 2, 4, 8, 16, 32):
                other = np.zeros_like(u)
                other[:, :64 - d] = u[:, d:]
                hd_other = np.full(64, -2)
                hd_other[:64 - d] = hd[d:]
                take = (lanes + d < 64) & (hd >= 0) & (hd_other == hd)
                u = np.where(take[None, :], u + other, u).astype(f32)
            folded.append(u)
        for h in range(c0 // C, (c_end - 1) // C + 1):
            lo, hi = max(h * C, c0), min((h + 1) * C, c_end)
            if C % 4 == 0:
                part = folded[0][:, (lo - c0) >> 2]
            else:
                p = []
                for k in range(4):
                    c1 = lo + ((k - lo) & 3)
                    p.append(folded[k][:, (c1 - c0) >> 2] if c1 < hi else np.zeros(T, dtype=f32))
                part = ((p[0] + p[1]) + p[2]) + p[3]
            e[:, h] = part if h * C >= c0 else e[:, h] + part
    return e


def e_restatement(hl, hr, att, src, dst, slope) -> np.ndarray:
    """e [T, H] float32 of the terms (src[t] -> dst[t]): hl, hr [n, H, C], att [H, C]."""
    f32 = np.float32
    hl, hr, att = (np.asarray(a, dtype=f32) for a in (hl, hr, att))
    _, H, C = hl.shape
    z = hl[src].reshape(-1, H * C) + hr[dst].reshape(-1, H * C)
    lk = np.where(z > 0, z, f32(slope) * z).astype(f32)
    return fold_restatement(att.reshape(1, H * C) * lk, H, C)


def dot_restatement(g, hl, src, dst) -> np.ndarray:
    """dalpha [T, H] float32 in the same order: the term is g[dst] * hl[src]."""
    g, hl = np.asarray(g, dtype=np.float32), np.asarray(hl, dtype=np.float32)
    _, H, C = hl.shape
    return fold_restatement(g[dst].reshape(-1, H * C) * hl[src].reshape(-1, H * C), H, C)


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
    share_weights: bool = False
    graph: str = "main"

    @property
    def id(self):
        tags = [f"{self.c_in}x{self.H}x{self.C}"] + [t for t, on in (("mean", not self.concat), ("nobias", not self.bias),
                                                                     ("nogradx", not self.grad_x), ("noself", not self.add_self_loops),
                                                                     ("slope0", self.negative_slope == 0.0), ("overflow", self.att_scale != 1.0),
                                                                     ("shared", self.share_weights)) if on]
        return "-".join(tags)

    @property
    def width(self):
        return self.H * self.C if self.concat else self.C

    @property
    def param_keys(self):
        keys = ["lin_l.weight"] + (["lin_l.bias"] if self.bias else [])
        if not self.share_weights:
            keys += ["lin_r.weight"] + (["lin_r.bias"] if self.bias else [])
        return tuple(keys + ["att"] + (["bias"] if self.bias else []))


SHAPES = ((36, 1, 64), (36, 4, 64), (36, 8, 8), (12, 3, 7), (36, 2, 130), (37, 1, 5), (12, 5, 1), (12, 1, 260), (12, 3, 100))
OVERFLOW_CASE = LayerCase(36, 4, 64, att_scale=400.0)
SHARED_CASE = LayerCase(36, 4, 64, share_weights=True)
LAYER_CASES = tuple(LayerCase(*s) for s in SHAPES) + (
    LayerCase(36, 4, 64, concat=False), LayerCase(36, 4, 64, bias=False), LayerCase(36, 4, 64, grad_x=False),
    LayerCase(36, 4, 64, add_self_loops=False), LayerCase(36, 4, 64, negative_slope=0.0), SHARED_CASE, OVERFLOW_CASE,
    LayerCase(12, 3, 7, concat=False))


@functools.lru_cache(maxsize=None)
def layer_inputs(case: LayerCase):
    """float32 arrays: x, the two linear layers, att [1, H, C], bias, and the upstream gradient g (loss = sum(out * g))."""
    g = graph(case.graph)
    rs = np.random.RandomState(7000 + 17 * case.c_in + 101 * case.H + case.C)
    bound = 1.0 / np.sqrt(case.c_in)
    a = case.att_scale / np.sqrt(case.C)
    HC = case.H * case.C
    return {"x": (0.25 + rs.randn(g.n, case.c_in)).astype(np.float32),
            "lin_l.weight": rs.uniform(-bound, bound, size=(HC, case.c_in)).astype(np.float32),
            "lin_l.bias": rs.uniform(-bound, bound, size=HC).astype(np.float32),
            "lin_r.weight": rs.uniform(-bound, bound, size=(HC, case.c_in)).astype(np.float32),
            "lin_r.bias": rs.uniform(-bound, bound, size=HC).astype(np.float32),
            "att": (a * rs.randn(1, case.H, case.C)).astype(np.float32),
            "bias": rs.uniform(-bound, bound, size=case.width).astype(np.float32),
            "g": rs.randn(g.n, case.width).astype(np.float32)}


def _project(x, p, H, C):
    """hl, hr [n, H, C] from the parameter dict p (lin_r.* absent: shared weights; biases absent: none)."""
    n = x.shape[0]
    hl = F.linear(x, p["lin_l.weight"], p.get("lin_l.bias")).view(n, H, C)
    hr = F.linear(x, p["lin_r.weight"], p.get("lin_r.bias")).view(n, H, C) if "lin_r.weight" in p else hl
    return hl, hr


def _finish(agg, bias, concat):
    n, H, C = agg.shape
    out = agg.reshape(n, H * C) if concat else agg.sum(1) / H
    return out if bias is None else out + bias


def dense_layer(name, x, p, H, C, concat, slope, self_loops, pattern=None):
    """-> (out, w [H, n, n] detached: M_ij alpha_ij).  pattern: bool [n, n, H, C] indexed [i, j] (z > 0 where None)."""
    m_ = multiplicity(name, self_loops).to(x.dtype)
    n = x.shape[0]
    hl, hr = _project(x, p, H, C)
    att = p["att"].view(H, C)
    heads, ws = [], []
    for k in range(H):
        blocks, wk = [], []
        for r0 in range(0, n, ROW_BLOCK):
            rows = slice(r0, min(n, r0 + ROW_BLOCK))
            z = hl[None, :, k, :] + hr[rows, None, k, :]                                    # [B, n, C]
            pat = (z.detach() > 0) if pattern is None else pattern[rows, :, k, :]
            e = (torch.where(pat, z, slope * z) * att[k]).sum(-1)                           # [B, n]
            mb = m_[rows]
            em = e.masked_fill(~(mb > 0), float("-inf"))
            top = em.detach().max(dim=1, keepdim=True).values
            top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
            ex = torch.exp(em - top) * mb
            s = ex.sum(1, keepdim=True)
            w = ex / torch.where(s > 0, s, torch.ones_like(s))
            blocks.append(w @ hl[:, k, :])
            wk.append(w.detach())
        heads.append(torch.cat(blocks, 0))
        ws.append(torch.cat(wk, 0))
    agg = torch.stack(heads, 1)
    return _finish(agg, p.get("bias"), concat), torch.stack(ws, 0)


def edge_layer(name, x, p, H, C, concat, slope, self_loops, perm_seed, pattern=None):
    """The layer edge by edge in x's dtype, stock torch ops over the (permuted) term list."""
    src, dst = gc._edges(name, self_loops, perm_seed)
    n = x.shape[0]
    hl, hr = _project(x, p, H, C)
    if src.numel() == 0:
        return _finish(torch.zeros_like(hl) * hl, p.get("bias"), concat)
    z = hl.index_select(0, src) + hr.index_select(0, dst)                                   # [E, H, C]
    pat = (z.detach() > 0) if pattern is None else pattern[dst, src]
    e = (torch.where(pat, z, slope * z) * p["att"].view(1, H, C)).sum(-1)                   # [E, H]
    idx = dst[:, None].expand(-1, H)
    top = torch.full((n, H), float("-inf"), dtype=x.dtype).scatter_reduce(0, idx, e.detach(), "amax", include_self=True)
    ex = torch.exp(e - top.index_select(0, dst))
    s = torch.zeros((n, H), dtype=x.dtype).index_add_(0, dst, ex)
    alpha = ex / s.index_select(0, dst)
    agg = torch.zeros_like(hl).index_add_(0, dst, alpha[:, :, None] * hl.index_select(0, src))
    return _finish(agg, p.get("bias"), concat)


def _layer_tensors(case: LayerCase, forward, dtype):
    """out and the gradients of sum(out * g) as a dict of tensors."""
    t = {k: torch.from_numpy(v).to(dtype) for k, v in layer_inputs(case).items()}
    x = t["x"].requires_grad_(True)
    p = {k: t[k].requires_grad_(True) for k in case.param_keys}
    out = forward(x, p)
    (out * t["g"]).sum().backward()
    got = {"out": out.detach(), "grad_x": x.grad}
    got.update({"grad_" + k: v.grad for k, v in p.items()})
    return got


def _conf(case: LayerCase):
    return case.H, case.C, case.concat, case.negative_slope, case.add_self_loops


def _z64(case: LayerCase, rows):
    t = {k: torch.from_numpy(v).double() for k, v in layer_inputs(case).items()}
    hl, hr = _project(t["x"], {k: t[k] for k in case.param_keys}, case.H, case.C)
    return hl[None, :] + hr[rows, None]                                                     # [B, n, H, C]


@functools.lru_cache(maxsize=None)
def layer_gate(case: LayerCase):
    """(pattern_64 bool [n, n, H, C] indexed [i, j], terms bool [n, n], gated bool [n, n, H, C]) of the unresolved float64 reference."""
    n = graph(case.graph).n
    terms = multiplicity(case.graph, case.add_self_loops) > 0
    count, total, squares = 0, 0.0, 0.0
    for r0 in range(0, n, ROW_BLOCK):
        rows = slice(r0, min(n, r0 + ROW_BLOCK))
        z = _z64(case, rows)[terms[rows]]
        count, total, squares = count + z.numel(), total + float(z.sum()), squares + float((z * z).sum())
    std = np.sqrt(max(squares - total * total / count, 0.0) / (count - 1)) if count > 1 else 0.0
    pattern = torch.zeros((n, n, case.H, case.C), dtype=torch.bool)
    gated = torch.zeros_like(pattern)
    for r0 in range(0, n, ROW_BLOCK):
        rows = slice(r0, min(n, r0 + ROW_BLOCK))
        z = _z64(case, rows)
        pattern[rows] = z > 0
        gated[rows] = (z.abs() < GATE * std) & terms[rows][:, :, None, None]
    return pattern, terms, gated


def gate_share(case: LayerCase) -> float:
    _, terms, gated = layer_gate(case)
    return float(gated.sum()) / max(float(terms.sum()) * case.H * case.C, 1.0)


def device_pattern(hl, hr, H, C) -> torch.Tensor:
    """bool [n, n, H, C] indexed [i, j] from the device's float32 hl, hr [n, H C]: (hl[j] + hr[i]) > 0, the sum in float32."""
    hl, hr = hl.float().cpu(), hr.float().cpu()
    n = hl.shape[0]
    return ((hl[None, :, :] + hr[:, None, :]) > 0).view(n, n, H, C)


def resolve_pattern(case: LayerCase, device_on=None):
    """(pattern, gated count, mismatches): the reference's pattern with the device's inside the gate; mismatches: elements of terms
    outside the gate where the device's pattern differs."""
    pattern, terms, gated = layer_gate(case)
    mismatches = None
    if device_on is not None:
        mismatches = int(((device_on != pattern) & terms[:, :, None, None] & ~gated).sum())
        pattern = torch.where(gated, device_on, pattern)
    return pattern, int(gated.sum()), mismatches


def _bias_grad_draws(g):
    g = torch.from_numpy(g)
    draws = []
    for k in range(PERMS):
        p = torch.from_numpy(np.random.RandomState(1300 + k).permutation(g.shape[0]))
        draws.append(g.index_select(0, p).sum(0))
        acc = torch.zeros(g.shape[1])
        for r in p.tolist():
            acc = acc + g[r]
        draws.append(acc)
    return draws


_EXPECT = {}


def layer_expectation(case: LayerCase, device_on=None):
    """(T_64, err_32, gated, mismatches): the reference under the resolved pattern and, per tensor, the largest error of the float32
    restatements under the same pattern.  Computed once per (case, pattern inside the gate)."""
    pattern, n_gated, mismatches = resolve_pattern(case, device_on)
    _, _, gated = layer_gate(case)
    key = (case, tuple(pattern[gated].tolist()))
    if key not in _EXPECT:
        conf = _conf(case)
        t64 = _layer_tensors(case, lambda x, p: dense_layer(case.graph, x, p, *conf, pattern=pattern)[0], torch.float64)
        err32 = {k: 0.0 for k in t64}
        for perm in (None, *range(PERMS)):
            got = _layer_tensors(case, lambda x, p: edge_layer(case.graph, x, p, *conf, perm, pattern=pattern), torch.float32)
            for k in t64:
                err32[k] = max(err32[k], err(got[k], t64[k]))
        if case.bias:
            err32["grad_bias"] = max([err32["grad_bias"]] + [err(d, t64["grad_bias"]) for d in _bias_grad_draws(layer_inputs(case)["g"])])
        _EXPECT[key] = (t64, err32)
    return (*_EXPECT[key], n_gated, mismatches)


def slot_alpha(case: LayerCase, dtype=torch.float64, pattern=None):
    """(alpha [nnz, H], alpha_self [n, H]) of the dense formula in `dtype` under `pattern` (None: its own), in the slot order of
    canonical(by destination)."""
    t = {k: torch.from_numpy(v).to(dtype) for k, v in layer_inputs(case).items()}
    with torch.no_grad():
        _, w = dense_layer(case.graph, t["x"], {k: t[k] for k in case.param_keys}, *_conf(case), pattern=pattern)
    m_ = multiplicity(case.graph, case.add_self_loops).to(dtype)
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
        alpha_self = torch.zeros((g.n, case.H), dtype=dtype)
    return alpha, alpha_self


@functools.lru_cache(maxsize=None)
def reference_alpha(case: LayerCase):
    """slot_alpha of the unresolved float64 reference."""
    return slot_alpha(case)


def alpha_expectation(case: LayerCase, device_on):
    """(alpha_64, alpha_self_64, err_32): the reference's attention under the resolved pattern (the device's inside the gate) and the
    error of the dense formula run in float32 under the same pattern, the restatement the rule asks for."""
    pattern, _, _ = resolve_pattern(case, device_on)
    ref, ref_self = slot_alpha(case, torch.float64, pattern)
    draw, draw_self = slot_alpha(case, torch.float32, pattern)
    return ref, ref_self, max(err(draw, ref), err(draw_self, ref_self) if case.add_self_loops else 0.0)


# ------------------------------------------------------------------------------------------------ the two-layer model

MODEL_IN, MODEL_HIDDEN, MODEL_OUT, MODEL_HEADS = gc.MODEL_IN, gc.MODEL_HIDDEN, gc.MODEL_OUT, gc.MODEL_HEADS
MODEL_LAYERS = gc.MODEL_LAYERS
PARAM_KEYS = ("lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "att", "bias")
PARAMS = tuple(f"convs.{i}.{k}" for i in range(2) for k in PARAM_KEYS)


@functools.lru_cache(maxsize=None)
def model_inputs():
    g = graph("main")
    rs = np.random.RandomState(79)
    t = {"x": (0.25 + rs.randn(g.n, MODEL_IN)).astype(np.float32), "y": rs.randint(0, MODEL_OUT, size=g.n).astype(np.int64)}
    for i, (ci, H, C) in enumerate(MODEL_LAYERS):
        bound = 1.0 / np.sqrt(ci)
        for side in "lr":
            t[f"convs.{i}.lin_{side}.weight"] = rs.uniform(-bound, bound, size=(H * C, ci)).astype(np.float32)
            t[f"convs.{i}.lin_{side}.bias"] = rs.uniform(-bound, bound, size=H * C).astype(np.float32)
        t[f"convs.{i}.att"] = (rs.randn(1, H, C) / np.sqrt(C)).astype(np.float32)
        t[f"convs.{i}.bias"] = rs.uniform(-bound, bound, size=H * C).astype(np.float32)
    return t


def model_run(dtype, patterns=(None, None), perm="dense"):
    """GATv2(36, 64, 5, heads=8) at dropout 0 + F.cross_entropy over all rows.  perm "dense": the dense formula; else the edge form under
    that permutation.  patterns: per layer the LeakyReLU pattern bool [n, n, H, C] or None.  -> dict: z0, z1 (hl, hr of each layer,
    detached), logits, loss, grad:<param>."""
    t = model_inputs()
    p = {k: torch.from_numpy(t[k]).to(dtype).requires_grad_(True) for k in PARAMS}
    h, y = torch.from_numpy(t["x"]).to(dtype), torch.from_numpy(t["y"])
    out = {}
    for i, (_, H, C) in enumerate(MODEL_LAYERS):
        pi = {k: p[f"convs.{i}.{k}"] for k in PARAM_KEYS}
        out[f"z{i}"] = tuple(a.detach() for a in _project(h, pi, H, C))
        if perm == "dense":
            h, _ = dense_layer("main", h, pi, H, C, True, 0.2, True, pattern=patterns[i])
        else:
            h = edge_layer("main", h, pi, H, C, True, 0.2, True, perm, pattern=patterns[i])
        if i == 0:
            h = F.elu(h)
    loss = F.cross_entropy(h, y)
    loss.backward()
    out.update({"logits": h.detach(), "loss": float(loss.detach())})
    out.update({"grad:" + k: v.grad for k, v in p.items()})
    return out


@functools.lru_cache(maxsize=None)
def model_gate():
    """Per layer (pattern_64, terms, gated) of the unresolved float64 model."""
    ref = model_run(torch.float64)
    terms = multiplicity("main", True) > 0
    gates = []
    for i in range(2):
        hl, hr = ref[f"z{i}"]
        z = hl[None, :] + hr[:, None]                                                       # [n, n, H, C]
        gated = (z.abs() < GATE * float(z[terms].std())) & terms[:, :, None, None]
        gates.append((z > 0, terms, gated))
    return gates


def model_expectation(device_on=None):
    """(ref, err_32, gated share, mismatches): the float64 model under the resolved patterns (the device's inside the gates), the
    restatements' errors under the same patterns."""
    patterns, n_gated, n_elems, mismatches = [], 0, 0, None if device_on is None else 0
    for i, (pat, terms, gated) in enumerate(model_gate()):
        if device_on is not None:
            mismatches += int(((device_on[i] != pat) & terms[:, :, None, None] & ~gated).sum())
            pat = torch.where(gated, device_on[i], pat)
        patterns.append(pat)
        n_gated += int(gated.sum())
        n_elems += int(terms.sum()) * pat.shape[2] * pat.shape[3]
    ref = model_run(torch.float64, patterns)
    err32 = {k: 0.0 for k in ref if k == "logits" or k.startswith("grad:")}
    for perm in (None, *range(PERMS)):
        got = model_run(torch.float32, patterns, perm)
        for k in err32:
            err32[k] = max(err32[k], err(got[k], ref[k]))
    return ref, err32, n_gated / n_elems, mismatches
