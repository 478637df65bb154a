"""Cases, float64 reference, float32 restatements and the threshold for GCNConv / GCN on the whole graph (include/graphpope_hip.h:
pope_gcn_*; graphpope_amd/gcn.py).  Imports without a GPU and is not a test module: test_gcn_cpu.py proves the reference, the graph and
the threshold on the CPU, test_gcn_gpu.py runs the kernels through them.

Graph: full_inference_cases.graph("main") (300 nodes, 4 029 slots, 58 self-loops, repeated edges, directed; row degrees 0 .. 1 025, so
the hub path and both of its edges are in it) and its degenerate siblings "single" (N = 1, no edge) and "empty" (N = 17, every row empty).
:func:`transposed` is the CSR by source, rows ascending, as engine.build_csr_canonical builds it.

Reference (:func:`dense_adjacency` / :func:`dense_layer`): the dense formula  out = D^-1/2 (A + f I) D^-1/2 x W + b  in float64 under autograd, A built from
the slot list (repeated edges add up; with a self weight the diagonal is REPLACED by f).  It shares no structure with the kernels.
Restatement (:func:`edge_layer`): float32, edge by edge with index_add_, in both association orders (project-first, aggregate-first)
and under PERMS permutations of the edge order; for the bias gradient the rows of grad_out are permuted as well (torch's column sum in
one order is a single draw).

Error measure: err(T) = max |T - T_64| / max |T_64|.
Threshold: err_dev <= FACTOR * max(err_32, 2^-23), FACTOR = 4 and PERMS = 6: the rule of sage_model_cases.py (2 for a second draw of the
same rounding process, 2 for the kernels' different but equally legitimate summation structure: MFMA tiles, split depth, chunked hub sums).

Documented order (:func:`propagate_restatement`): NumPy float32, operation by operation, what the header's summation contract says; the
device must give these bits.

Model (:func:`model_run`): a two-layer GCN at dropout 0 with F.cross_entropy over all rows.  ReLU gate as in sage_model_cases.py: the
hidden pre-activation is not normalised here, so an element is gated when |z_64| < GATE * std(z_64); there the reference takes the
pattern the device produced, outside it the device's pattern must equal the reference's.  The gated share is at most
bn_epilogue_cases.EXCLUDED_CAP.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import bn_epilogue_cases as bn
import full_inference_cases as fic

CHUNK = fic.CHUNK
PERMS = 6
FACTOR = 4.0
FLOOR = 2.0 ** -23
GATE = 2.0 ** -12
CUS = 256

SHAPES = ((36, 256), (36, 260), (12, 7), (256, 512), (37, 64))
WHOLE_TILE_SHAPE = (36, 640)           # the smallest kind of shape at which 300 rows take the whole-tile projection (test_gcn_cpu.py: the names)
PROPAGATE_WIDTHS = (7, 64, 256, 260, 512)
SETTINGS = ((False, True), (True, True), (False, False), (True, False))        # (improved, add_self_loops)
MODEL_IN, MODEL_HIDDEN, MODEL_OUT = 36, 64, 5

graph = fic.graph
err = fic.err


def self_weight(improved: bool, add_self_loops: bool) -> float:
    return (2.0 if improved else 1.0) if add_self_loops else 0.0


@functools.lru_cache(maxsize=None)
def transposed(name: str = "main"):
    """(rowptr_t, col_t) int32: the CSR by source of graph(name), every row ascending (repeated edges adjacent)."""
    g = graph(name)
    src, dst = g.src, g.dst
    order = np.lexsort((dst, src))
    rowptr = np.zeros(g.n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(src, minlength=g.n))
    return rowptr.astype(np.int32), dst[order].astype(np.int32)


def csr(name: str, by_source: bool):
    g = graph(name)
    return transposed(name) if by_source else (g.rowptr, g.col)


# ------------------------------------------------------------------------------------------------ the documented order, bit for bit

def dinv_restatement(rowptr, col, n, f: float) -> np.ndarray:
    """float32 [n]: (float)(1 / sqrt((double)deg)), deg = the row's slots (with f > 0: those whose id is not the row) + f; 0 for deg 0."""
    out = np.zeros(n, dtype=np.float32)
    for i in range(n):
        ids = col[rowptr[i]:rowptr[i + 1]]
        deg = np.float64(int((ids != i).sum()) if f > 0 else ids.size) + np.float64(np.float32(f))
        out[i] = np.float32(1.0 / np.sqrt(deg)) if deg > 0 else np.float32(0.0)
    return out


def propagate_restatement(rowptr, col, n, h, dinv=None, f: float = 0.0, bias=None) -> np.ndarray:
    """out [n, C] float32 in the order include/graphpope_hip.h documents: every product and every sum a float32 operation of its own."""
    f32 = np.float32
    h = np.asarray(h, dtype=f32)
    out = np.zeros_like(h)
    zero = np.zeros(h.shape[1], dtype=f32)
    for i in range(n):
        beg, end = int(rowptr[i]), int(rowptr[i + 1])

        def run(lo, hi):
            s = zero.copy()
            for p in range(lo, hi):
                j = int(col[p])
                if j < 0 or j >= n or (f > 0 and j == i):
                    continue
                s = s + (h[j] if dinv is None else (dinv[j] * h[j]).astype(f32))
            return s

        if end - beg <= CHUNK:
            s = run(beg, end)
        else:
            s = zero.copy()
            for lo in range(beg, end, CHUNK):                       # runs of CHUNK slot positions, skipped slots included
                s = s + run(lo, min(lo + CHUNK, end))
        if f > 0:
            sw = f32(f) if dinv is None else f32(dinv[i] * f32(f))
            s = s + (sw * h[i]).astype(f32)
        if dinv is not None:
            s = (dinv[i] * s).astype(f32)
        if bias is not None:
            s = s + np.asarray(bias, dtype=f32)
        out[i] = s
    return out


# ------------------------------------------------------------------------------------------------ layer cases

@dataclass(frozen=True)
class LayerCase:
    c_in: int
    c_out: int
    bias: bool = True
    grad_x: bool = True
    normalize: bool = True
    improved: bool = False
    add_self_loops: bool = True
    graph: str = "main"

    @property
    def id(self):
        tags = [f"{self.c_in}x{self.c_out}"] + [t for t, on in (("nobias", not self.bias), ("nogradx", not self.grad_x), ("plain", not self.normalize),
                                                                ("improved", self.improved), ("noself", not self.add_self_loops)) if on]
        return "-".join(tags)

    @property
    def f(self):
        return self_weight(self.improved, self.add_self_loops) if self.normalize else 0.0


LAYER_CASES = tuple(LayerCase(ci, co) for ci, co in SHAPES + (WHOLE_TILE_SHAPE,)) + (
    LayerCase(36, 256, bias=False), LayerCase(36, 256, grad_x=False), LayerCase(37, 64, bias=False, grad_x=False),
    LayerCase(36, 256, normalize=False), LayerCase(36, 260, improved=True), LayerCase(12, 7, add_self_loops=False))


@functools.lru_cache(maxsize=None)
def layer_inputs(case: LayerCase):
    """float32 arrays: x, weight [c_in, c_out], bias, and the upstream gradient g [n, c_out] (loss = sum(out * g))."""
    g = graph(case.graph)
    rs = np.random.RandomState(4000 + 17 * case.c_in + case.c_out)
    bound = 1.0 / np.sqrt(case.c_in)
    return {"x": (0.25 + rs.randn(g.n, case.c_in)).astype(np.float32),
            "weight": rs.uniform(-bound, bound, size=(case.c_in, case.c_out)).astype(np.float32),
            "bias": rs.uniform(-bound, bound, size=case.c_out).astype(np.float32),
            "g": rs.randn(g.n, case.c_out).astype(np.float32)}


def _edges(name, perm_seed):
    g = graph(name)
    src, dst = g.src, g.dst
    if perm_seed is not None and src.size:
        p = np.random.RandomState(900 + perm_seed).permutation(src.size)
        src, dst = src[p], dst[p]
    return torch.from_numpy(src), torch.from_numpy(dst)


def dense_adjacency(name: str, normalize: bool, f: float) -> torch.Tensor:
    """float64 [n, n]: D^-1/2 (A + f I) D^-1/2 (normalize), or A itself; A[i, j] = how often row i holds j."""
    g = graph(name)
    a = torch.zeros((g.n, g.n), dtype=torch.float64)
    src, dst = _edges(name, None)
    a.index_put_((dst, src), torch.ones(src.numel(), dtype=torch.float64), accumulate=True)
    if not normalize:
        return a
    if f > 0:
        a.fill_diagonal_(f)
    deg = a.sum(1)
    dinv = torch.where(deg > 0, deg.clamp(min=1e-300).pow(-0.5), torch.zeros_like(deg))
    return dinv[:, None] * a * dinv[None, :]


def dense_layer(a_hat, x, weight, bias):
    out = a_hat @ x @ weight
    return out if bias is None else out + bias


def edge_layer(name, x, weight, bias, normalize, f, order, perm_seed):
    """The layer edge by edge in x's dtype: index_add_ over the (permuted) edge list, the self term on its own."""
    g = graph(name)
    src, dst = _edges(name, perm_seed)
    dt = x.dtype
    if normalize:
        keep = src != dst if f > 0 else torch.ones_like(src, dtype=torch.bool)
        src, dst = src[keep], dst[keep]
        deg = torch.bincount(dst, minlength=g.n).to(dt) + f
        dinv = torch.where(deg > 0, deg.clamp(min=1e-30).pow(-0.5), torch.zeros_like(deg))
        w = (dinv[src] * dinv[dst])[:, None]
        own = (dinv * dinv * f)[:, None]
    else:
        w, own = None, None

    def spread(h):
        msg = h.index_select(0, src)
        out = torch.zeros_like(h).index_add_(0, dst, msg if w is None else msg * w)
        return out if own is None or f == 0 else out + own * h

    out = spread(x @ weight) if order == "project" else spread(x) @ weight
    return out if bias is None else out + bias


def _layer_tensors(case: LayerCase, forward, dtype):
    """out and the gradients of sum(out * g) as a dict of tensors."""
    t = {k: torch.from_numpy(v).to(dtype) for k, v in layer_inputs(case).items()}
    x, w = t["x"].requires_grad_(True), t["weight"].requires_grad_(True)
    b = t["bias"].requires_grad_(True) if case.bias else None
    out = forward(x, w, b)
    (out * t["g"]).sum().backward()
    got = {"out": out.detach(), "grad_x": x.grad, "grad_weight": w.grad}
    if case.bias:
        got["grad_bias"] = b.grad
    return got


def _bias_grad_draws(case: LayerCase):
    """The float32 column sums of g under PERMS row orders: further draws of the bias gradient's rounding."""
    g = torch.from_numpy(layer_inputs(case)["g"])
    draws = []
    for k in range(PERMS):
        p = torch.from_numpy(np.random.RandomState(1300 + k).permutation(g.shape[0]))
        draws.append(g.index_select(0, p).sum(0))
        acc = torch.zeros(g.shape[1])
        for r in p.tolist():                                          # ... and the plain sequential sum in that order
            acc = acc + g[r]
        draws.append(acc)
    return draws


@functools.lru_cache(maxsize=None)
def layer_expectation(case: LayerCase):
    """(T_64, err_32): the reference tensors and, per tensor, the largest error of the float32 restatements.  Computed once per case."""
    a_hat = dense_adjacency(case.graph, case.normalize, case.f)
    t64 = _layer_tensors(case, lambda x, w, b: dense_layer(a_hat, x, w, b), torch.float64)
    err32 = {k: 0.0 for k in t64}
    for order in ("project", "aggregate"):
        for perm in (None, *range(PERMS)):
            got = _layer_tensors(case, lambda x, w, b: edge_layer(case.graph, x, w, b, case.normalize, case.f, order, perm), torch.float32)
            for k in t64:
                err32[k] = max(err32[k], err(got[k], t64[k]))
    if case.bias:
        err32["grad_bias"] = max([err32["grad_bias"]] + [err(d, t64["grad_bias"]) for d in _bias_grad_draws(case)])
    return t64, err32


def threshold(err32: float) -> float:
    return FACTOR * max(err32, FLOOR)


# ------------------------------------------------------------------------------------------------ the two-layer model

@functools.lru_cache(maxsize=None)
def model_inputs():
    g = graph("main")
    rs = np.random.RandomState(77)
    t = {"x": (0.25 + rs.randn(g.n, MODEL_IN)).astype(np.float32), "y": rs.randint(0, MODEL_OUT, size=g.n).astype(np.int64)}
    for i, (ci, co) in enumerate(((MODEL_IN, MODEL_HIDDEN), (MODEL_HIDDEN, MODEL_OUT))):
        bound = 1.0 / np.sqrt(ci)
        t[f"convs.{i}.weight"] = rs.uniform(-bound, bound, size=(ci, co)).astype(np.float32)
        t[f"convs.{i}.bias"] = rs.uniform(-bound, bound, size=co).astype(np.float32)
    return t


PARAMS = ("convs.0.weight", "convs.0.bias", "convs.1.weight", "convs.1.bias")


def model_run(dtype, pattern=None, order=None, perm=None):
    """GCN(36, 64, 5) at dropout 0 + F.cross_entropy over all rows.  order None: the dense float64-style formula; else the edge form.
    pattern: the ReLU's pattern (bool [n, hidden]), or None for z > 0.  -> dict: z (hidden pre-activation), logits, loss, grad:<param>."""
    t = model_inputs()
    p = {k: torch.from_numpy(t[k]).to(dtype).requires_grad_(True) for k in PARAMS}
    x, y = torch.from_numpy(t["x"]).to(dtype), torch.from_numpy(t["y"])
    if order is None:
        a_hat = dense_adjacency("main", True, 1.0).to(dtype)
        conv = lambda h, i: dense_layer(a_hat, h, p[f"convs.{i}.weight"], p[f"convs.{i}.bias"])                       # noqa: E731
    else:
        conv = lambda h, i: edge_layer("main", h, p[f"convs.{i}.weight"], p[f"convs.{i}.bias"], True, 1.0, order, perm)  # noqa: E731
    z = conv(x, 0)
    on = (z.detach() > 0) if pattern is None else pattern
    logits = conv(z * on.to(dtype), 1)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    out = {"z": z.detach(), "logits": logits.detach(), "loss": float(loss.detach())}
    out.update({"grad:" + k: v.grad for k, v in p.items()})
    return out


def model_gate():
    """(z_64, gated): the reference's hidden pre-activation and the elements within GATE * std of zero."""
    z = model_run(torch.float64)["z"]
    return z, z.abs() < GATE * float(z.std())


def model_expectation(device_on=None):
    """(ref, err_32, gated, mismatches): the float64 run under the resolved pattern (the device's inside the gate), the restatements'
    errors under the same pattern, the gated count and, with a device pattern, the elements outside the gate where it differs."""
    z, gated = model_gate()
    pattern = z > 0
    mismatches = None
    if device_on is not None:
        mismatches = int(((device_on != pattern) & ~gated).sum())
        pattern = torch.where(gated, device_on, pattern)
    ref = model_run(torch.float64, pattern)
    err32 = {k: 0.0 for k in ref if k not in ("loss", "z")}
    for order in ("project", "aggregate"):
        for perm in (None, *range(PERMS)):
            got = model_run(torch.float32, pattern, order, perm)
            for k in err32:
                err32[k] = max(err32[k], err(got[k], ref[k]))
    return ref, err32, int(gated.sum()), mismatches


def loss_bound(ref, err32) -> float:
    """sage_model_cases.py's rule: 2 * (allowed absolute logits error) + 8 * 2^-24 * max |logits_64|."""
    top = float(ref["logits"].abs().max())
    return 2.0 * threshold(err32["logits"]) * top + 8.0 * 2.0 ** -24 * top


EXCLUDED_CAP = bn.EXCLUDED_CAP


# ------------------------------------------------------------------------------------------------ the training smoke graph

def planted_partition(n=240, classes=3, seed=5):
    """(edge_index int64 [2, E], x float32 [n, 16], y int64 [n]): a symmetric planted-partition graph whose features carry a weak
    class signal; a GCN separates it in a few steps."""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, classes, size=n)
    same = y[:, None] == y[None, :]
    prob = np.where(same, 0.08, 0.005)
    upper = np.triu(rs.rand(n, n) < prob, 1)
    s, d = np.nonzero(upper | upper.T)
    x = (rs.randn(n, 16) + 0.5 * np.eye(classes, 16)[y]).astype(np.float32)
    return np.stack([s, d]).astype(np.int64), x, y.astype(np.int64)
