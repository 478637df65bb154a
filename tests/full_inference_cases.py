"""Cases, float64 reference, float32 restatements and the threshold for exact full-graph SAGE inference (include/graphpope_hip.h:
sage_full_layer_forward; graphpope_amd/sage.py: SAGE.inference).  Imports without a GPU and is not a test module:
test_full_inference_cpu.py proves the reference, the graph and the threshold on the CPU, test_full_inference_gpu.py runs the kernels
through them.

Graph (:func:`graph`): one directed multigraph of N = 300 nodes whose destination rows include each of the degrees DEGREES -- the unroll
remainders (0, 1, 3, 4, 5), the in-flight group (8, 9), the id batch (64, 65) and the hub path (CHUNK, CHUNK + 1, 2 CHUNK + 1).  N < CHUNK,
so the long rows are made of repeated edges; self-loops are present.  Every other row has 0 .. 12 slots.  The special rows are spread
over the node ids.  Degenerate graphs: N = 1 without an edge, N = 17 with every row empty.

Reference (:func:`layer_reference` / :func:`model_reference`): main.py:204-211 over the whole graph in plain torch, parameterised by
dtype, written aggregate-first: index_add_ over the edge list divided by max(deg, 1), two matmuls and a bias, then eval-mode BatchNorm
and ReLU on every layer but the last.  In float64 it is the reference.  In float32 it is the restatement, run in both association orders
(aggregate-first and project-first) and under PERMS permutations of the edge order.

Error measure: err(T) = max |T - T_64| / max |T_64|.
Threshold (:func:`layer_threshold` / :func:`model_threshold`): err_dev <= FACTOR * max(err_32 over both orders and all permutations, 2^-23),
computed from the reference side when the test runs.  FACTOR = 4 is the rule of sage_model_cases.py (2 for a second draw of the same
rounding process, 2 for the kernels' different but equally legitimate summation structure: MFMA tiles, chunked hub sums).  No ReLU gate
is needed: the forward value is continuous in the pre-activation.  The 2^-23 floor covers the degenerate graphs, whose restatement may
be exact.

Documented order (:func:`chunked_restatement`): NumPy float32, operation by operation, the summation order the header documents -- a row
of up to CHUNK slots in slot order, a longer one as runs of CHUNK slots whose sums are added in run order, then * 1/deg, + R, BatchNorm,
ReLU.  With identity weights the projection is exact and the device must give these bits.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch

CHUNK = 512                # test_full_inference_gpu.py asserts it against the value include/graphpope_hip.h documents
N = 300
DEGREES = (0, 1, 3, 4, 5, 8, 9, 64, 65, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
PERMS = 6
FACTOR = 4.0
FLOOR = 2.0 ** -23
EPS = float(np.float32(1e-5))
CUS = 256

SHAPES = ((36, 256), (36, 260), (12, 7), (256, 512), (37, 64))
GRAPHS = ("main", "single", "empty")
MODELS = ((2, 2), (3, 2), (3, 3))              # (num_layers, hops): hops <= the number of convs
MODEL_IN, MODEL_OUT, MODEL_HIDDEN = 36, 5, 64


# ------------------------------------------------------------------------------------------------ graphs

@dataclass(frozen=True)
class Graph:
    n: int
    rowptr: np.ndarray         # int32 [n + 1]
    col: np.ndarray            # int32 [nnz]: row v's slots hold the sources v aggregates, in slot order
    special: dict              # degree -> row, for every degree of DEGREES (main graph only)

    @property
    def nnz(self):
        return int(self.col.size)

    @property
    def dst(self):
        return np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.rowptr).astype(np.int64))

    @property
    def src(self):
        return self.col.astype(np.int64)


@functools.lru_cache(maxsize=None)
def graph(name: str = "main") -> Graph:
    if name == "single":
        return Graph(1, np.zeros(2, dtype=np.int32), np.zeros(0, dtype=np.int32), {})
    if name == "empty":
        return Graph(17, np.zeros(18, dtype=np.int32), np.zeros(0, dtype=np.int32), {})
    assert name == "main"
    rs = np.random.RandomState(20)
    deg = rs.randint(0, 13, size=N)
    rows = rs.permutation(N)[:len(DEGREES)]
    special = {}
    for d, v in zip(DEGREES, rows):
        deg[v] = d
        special[d] = int(v)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = rs.randint(0, N, size=int(rowptr[-1]))
    for v in range(0, N, 7):                                       # self-loops, in a middle slot of the row
        if deg[v] > 0:
            col[rowptr[v] + deg[v] // 2] = v
    for d in (4, 65, CHUNK + 1):                                   # ... and in rows of every kind
        v = special[d]
        col[rowptr[v]] = v
    return Graph(N, rowptr.astype(np.int32), col.astype(np.int32), special)


# ------------------------------------------------------------------------------------------------ layer cases

@dataclass(frozen=True)
class LayerCase:
    graph: str
    c_in: int
    c_out: int
    has_bn: bool

    @property
    def id(self):
        return f"{self.graph}-{self.c_in}x{self.c_out}-{'bn' if self.has_bn else 'plain'}"


LAYER_CASES = tuple(LayerCase("main", ci, co, bn) for ci, co in SHAPES for bn in (True, False)) + \
    tuple(LayerCase(g, 36, 256, bn) for g in ("single", "empty") for bn in (True, False))


def _bn_arrays(rs, c):
    """gamma, beta, running_mean (off-centre), running_var (1e-3 .. 1e3, both ends present)."""
    var = 10.0 ** rs.uniform(-3, 3, size=c)
    var[0] = 1e-3
    var[-1] = 1e3
    return {"gamma": rs.uniform(0.5, 1.5, size=c).astype(np.float32), "beta": (0.5 * rs.randn(c)).astype(np.float32),
            "mean": (0.3 + 0.5 * rs.randn(c)).astype(np.float32), "var": var.astype(np.float32)}


@functools.lru_cache(maxsize=None)
def layer_inputs(case: LayerCase):
    """float32 arrays of a layer case: x, w_l, b_l, w_r and, with BatchNorm, gamma / beta / mean / var."""
    g = graph(case.graph)
    rs = np.random.RandomState(1000 + 17 * case.c_in + case.c_out)
    bound = 1.0 / np.sqrt(case.c_in)
    t = {"x": (0.25 + rs.randn(g.n, case.c_in)).astype(np.float32),
         "w_l": rs.uniform(-bound, bound, size=(case.c_out, case.c_in)).astype(np.float32),
         "b_l": rs.uniform(-bound, bound, size=case.c_out).astype(np.float32),
         "w_r": rs.uniform(-bound, bound, size=(case.c_out, case.c_in)).astype(np.float32)}
    if case.has_bn:
        t.update(_bn_arrays(rs, case.c_out))
    return t


# ------------------------------------------------------------------------------------------------ reference and restatements

def _mean_aggregate(h, src, dst, n):
    """mean_{p in row v} h[src[p]] by index_add_ in the given edge order; an empty row gives 0."""
    agg = torch.zeros((n, h.shape[1]), dtype=h.dtype).index_add_(0, dst, h.index_select(0, src))
    deg = torch.bincount(dst, minlength=n).clamp(min=1).to(h.dtype)
    return agg / deg[:, None]


def _layer(h, src, dst, n, w_l, b_l, w_r, bn, order):
    if order == "aggregate":
        out = _mean_aggregate(h, src, dst, n) @ w_l.T + b_l + h @ w_r.T
    else:
        assert order == "project"
        out = _mean_aggregate(h @ w_l.T, src, dst, n) + b_l + h @ w_r.T
    if bn is not None:
        gamma, beta, mean, var = bn
        out = ((out - mean) / torch.sqrt(var + EPS) * gamma + beta).relu()
    return out


def _edges(g: Graph, perm_seed):
    src, dst = g.src, g.dst
    if perm_seed is not None and src.size:
        p = np.random.RandomState(500 + perm_seed).permutation(src.size)
        src, dst = src[p], dst[p]
    return torch.from_numpy(src), torch.from_numpy(dst)


def layer_reference(case: LayerCase, dtype=torch.float64, order="aggregate", perm_seed=None) -> torch.Tensor:
    g, t = graph(case.graph), {k: torch.from_numpy(v).to(dtype) for k, v in layer_inputs(case).items()}
    src, dst = _edges(g, perm_seed)
    bn = (t["gamma"], t["beta"], t["mean"], t["var"]) if case.has_bn else None
    return _layer(t["x"], src, dst, g.n, t["w_l"], t["b_l"], t["w_r"], bn, order)


def err(t, t64) -> float:
    """max |T - T_64| / max |T_64|."""
    t, t64 = torch.as_tensor(t).to(torch.float64), torch.as_tensor(t64).to(torch.float64)
    return float((t - t64).abs().max() / t64.abs().max())


def _restatement_error(run, t64):
    """The largest error of the float32 restatement over both association orders and the slot order plus PERMS edge permutations."""
    return max(err(run(torch.float32, order, perm), t64) for order in ("aggregate", "project") for perm in (None, *range(PERMS)))


@functools.lru_cache(maxsize=None)
def layer_expectation(case: LayerCase):
    """(T_64, err_32): the reference and the restatement's error, computed once per case and shared."""
    t64 = layer_reference(case)
    return t64, _restatement_error(lambda dtype, order, perm: layer_reference(case, dtype, order, perm), t64)


def layer_threshold(case: LayerCase) -> float:
    return FACTOR * max(layer_expectation(case)[1], FLOOR)


# ------------------------------------------------------------------------------------------------ model cases

@functools.lru_cache(maxsize=None)
def model_state(num_layers: int):
    """State dict (PyG names, float32 tensors) of SAGE(MODEL_IN, MODEL_OUT, MODEL_HIDDEN, num_layers): randomised weights, affine
    parameters and running statistics."""
    rs = np.random.RandomState(70 + num_layers)
    widths = [MODEL_IN] + [MODEL_HIDDEN] * (num_layers - 1) + [MODEL_OUT]
    state = {}
    for i in range(num_layers):
        c_in, c_out = widths[i], widths[i + 1]
        bound = 1.0 / np.sqrt(c_in)
        state[f"convs.{i}.lin_l.weight"] = rs.uniform(-bound, bound, size=(c_out, c_in)).astype(np.float32)
        state[f"convs.{i}.lin_l.bias"] = rs.uniform(-bound, bound, size=c_out).astype(np.float32)
        state[f"convs.{i}.lin_r.weight"] = rs.uniform(-bound, bound, size=(c_out, c_in)).astype(np.float32)
    for i in range(num_layers - 1):
        b = _bn_arrays(rs, MODEL_HIDDEN)
        state[f"bns.{i}.weight"], state[f"bns.{i}.bias"] = b["gamma"], b["beta"]
        state[f"bns.{i}.running_mean"], state[f"bns.{i}.running_var"] = b["mean"], b["var"]
        state[f"bns.{i}.num_batches_tracked"] = np.asarray(3, dtype=np.int64)
    return {k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}


@functools.lru_cache(maxsize=None)
def model_x():
    return (0.25 + np.random.RandomState(71).randn(N, MODEL_IN)).astype(np.float32)


def model_reference(num_layers: int, hops: int, dtype=torch.float64, order="aggregate", perm_seed=None) -> torch.Tensor:
    """SAGE.forward in eval mode over `hops` copies of the whole graph (main.py:204-211, the depth quirk included: with hops <
    num_layers the last conv never runs and the result is hidden-wide)."""
    g, state = graph("main"), model_state(num_layers)
    src, dst = _edges(g, perm_seed)
    h = torch.from_numpy(model_x()).to(dtype)
    for i in range(hops):
        bn = None
        if i < hops - 1:
            bn = tuple(state[f"bns.{i}.{k}"].to(dtype) for k in ("weight", "bias", "running_mean", "running_var"))
        h = _layer(h, src, dst, g.n, state[f"convs.{i}.lin_l.weight"].to(dtype), state[f"convs.{i}.lin_l.bias"].to(dtype),
                   state[f"convs.{i}.lin_r.weight"].to(dtype), bn, order)
    return h


@functools.lru_cache(maxsize=None)
def model_expectation(num_layers: int, hops: int):
    t64 = model_reference(num_layers, hops)
    return t64, _restatement_error(lambda dtype, order, perm: model_reference(num_layers, hops, dtype, order, perm), t64)


def model_threshold(num_layers: int, hops: int) -> float:
    return FACTOR * max(model_expectation(num_layers, hops)[1], FLOOR)


# ------------------------------------------------------------------------------------------------ the documented order, bit for bit

def chunked_restatement(g: Graph, p, r, bn=None) -> np.ndarray:
    """out [n, c] float32 from the projected rows p (gathered) and r (the row's own), in the order include/graphpope_hip.h documents:
    every operation a float32 operation of its own.  bn: (gamma, beta, mean, var) float32 arrays, or None."""
    f = np.float32
    p, r = np.asarray(p, dtype=f), np.asarray(r, dtype=f)
    out = np.zeros_like(r)
    if bn is not None:
        gamma, beta, mean, var = (np.asarray(a, dtype=f) for a in bn)
        rstd = (1.0 / np.sqrt(var.astype(np.float64) + np.float64(f(EPS)))).astype(f)
    for v in range(g.n):
        beg, end = int(g.rowptr[v]), int(g.rowptr[v + 1])
        deg = end - beg

        def run(lo, hi):
            s = np.zeros(p.shape[1], dtype=f)
            for q in range(lo, hi):
                s = s + p[g.col[q]]
            return s

        if deg <= CHUNK:
            s = run(beg, end)
        else:
            s = np.zeros(p.shape[1], dtype=f)
            for lo in range(beg, end, CHUNK):
                s = s + run(lo, min(lo + CHUNK, end))
        inv = f(1.0) / f(deg) if deg > 0 else f(0.0)
        t = (s * inv).astype(f) + r[v]
        if bn is not None:
            t = (((t - mean).astype(f) * rstd).astype(f) * gamma).astype(f) + beta
            t = np.where(t < 0, f(0.0), t).astype(f)
        out[v] = t
    return out
