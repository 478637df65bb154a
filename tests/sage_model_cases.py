"""Cases, float64 model, ReLU gate and thresholds for the composed GraphSAGE model (graphpope_amd/sage.py: SAGE.forward over the HIP
SAGEConv, BatchNorm/ReLU/dropout and cross-entropy kernels; graphpope_amd/train.py: SageTrainStep; graphpope_amd/optim.py: Adam).
Imports without a GPU and is not a test module: test_sage_model_cpu.py proves the reference and the thresholds on the CPU,
test_sage_model_gpu.py runs the kernels through them.

Reference (:func:`run_model`): SAGE.forward (main.py:204-211, the depth quirk included: one conv per sampled block, so the logits are
hidden_channels wide) followed by F.cross_entropy, in plain torch ops under autograd, parameterised by dtype.  Per block: mean
aggregation by index_add_ over the edge list divided by max(deg, 1); two matmuls and a bias; on every block but the last, batch
statistics with the biased variance, z = xhat * gamma + beta, y = z * pattern * mask / (1 - p), and the running statistics updated with
momentum 0.1 and the unbiased variance.  The mask is bn_epilogue_cases.keep_mask, the restatement of the kernels' counter hash.  In
float64 it is the reference; in float32 it is the "restatement" whose error against float64 is the yardstick.

Gate.  A float32 pre-activation within rounding of zero may fall on either side of the ReLU, and one such flip changes gradients by a
whole term.  Elements of a hidden layer whose reference |z| is below GATE = 2^-12 (z is normalised; the restatement's error in z is about
2^-20 of its scale) are gated: there the reference's backward pass uses the pattern the device produced -- the derivative of the function the
device computed.  Outside the gate the device's pattern must equal the reference's exactly.  The share of gated elements per layer is at most
bn_epilogue_cases.EXCLUDED_CAP.  Layers are resolved outer to inner: layer i + 1's z is computed from layer i's final pattern.

Comparison.  err(T) = max |T - T_64| / scale(T), scale(T) = max |T_64|, for the logits, every hidden y, every parameter gradient and the
running statistics.  One exception: the lin_l.bias gradient of a conv in front of a training-mode BatchNorm is zero in exact arithmetic
(BatchNorm removes what a bias adds), so its scale is max_c sum_r |grad_h_64[r, c]|, the sum whose cancellation produces it.
Threshold: err_dev(T) <= FACTOR * err_32(T), err_32 the restatement's error with the same pattern, the maximum over PERMS runs that permute
the order of the edges (the order of the additions in the aggregation and its transpose), computed from the reference side only when the
test runs.  FACTOR = 4: 2 for a second draw of the same rounding process (over such permutations max / median of a tensor's error
measured at most 2.0), 2 for the kernels' different but equally legitimate summation structure (split-K slabs, stream-K
cuts, atomics).
Loss: |loss - loss_64| <= 2 * (allowed absolute logits error) + 8 * 2^-24 * max |logits_64|.

Adam (:func:`adam_reference`): float64 Adam with step count k on (pre-step parameter, device gradient times the clip coefficient, pre-step
moments), compared element-wise within a bound from the float32 roundings of k_adam's documented formula (csrc/epilogue.hip):
    g' = g * coef;  m' = m + (g' - m)(1 - b1);  v' = b2 v + (1 - b2) g' g';  p' = p - step_size * (m' / (sqrt(v') * inv_bc2_sqrt + eps))
with step_size = float32(lr / (1 - b1^k)) and inv_bc2_sqrt = float32(1 / sqrt(1 - b2^k)).  Every operation and every float32 scalar counts
one ulp, U = 2^-23 relative (twice a correct rounding: first-order terms, the factor 2 covers the rest and a faithful rather than correct
division or square root); errors are propagated through the formulas, the square root by its exact interval.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

import bn_epilogue_cases as bn

GATE = 2.0 ** -12
FACTOR = 4.0
PERMS = 6
P = 0.5
CLASSES = 5
EPS = float(np.float32(bn.EPS))
MOMENTUM = float(np.float32(bn.MOMENTUM))
CUS = 256

DUAL = "k_gemm_dual<64, 64, 2, 2>[splits=%d]+k_scatter_and_finals"
STREAMK_TN = "k_gemm_streamk_tn<32>[xcd]+k_streamk_tn_fixup<32>"


def layer_seed(i: int) -> int:
    """The dropout seed SAGE.forward passes for hidden layer i when the seeds follow a device word."""
    return 0x9E3779B97F4A7C15 * (i + 1) % (1 << 63)


def drawn_seeds(manual_seed: int, hidden_layers: int):
    """The seeds SAGE.forward draws from torch's global generator (no device word) after torch.manual_seed(manual_seed)."""
    g = torch.Generator().manual_seed(manual_seed)
    return [int(torch.randint(0, 2 ** 62, (1,), generator=g).item()) for _ in range(hidden_layers)]


# ------------------------------------------------------------------------------------------------ cases

@dataclass(frozen=True)
class ModelCase:
    """A graph, a batch of seeds and a model.  `forward` / `backward`: per block, outer to inner, the kernels sage_forward_kernel_name /
    sage_backward_kernel_name must report on CUS compute units for (host-sized shapes, capacities of the device-extent batch): a table of
    outcomes, so that a retune which moves a case fails the pin.  `host_dims`: (n_dst, n_src) per block of the host-sized batch."""
    name: str
    graph: tuple                      # synth.powerlaw_graph arguments (n, pairs, seed, alpha, shift)
    first_seed: int
    batch: int
    sizes: tuple
    c_in: int
    hidden: int
    num_layers: int
    sample_seed: int
    host_dims: tuple
    forward: tuple
    backward: tuple
    bn_calls: tuple                   # per hidden layer, host-sized batch: True = the statistics hand-off runs


SMALL_GRAPH = (6000, 40000, 7, 0.9, 0.8)
BIG_GRAPH = (30000, 200000, 3, 0.62, 3.0)

CASES = {}


def _register(case):
    CASES[case.name] = case


_GENERIC = "k_gemm<64, 64, 2, 2, 0, 0>"
_VEC = "k_gemm<64, 64, 2, 2, 2, 2>"
_COLSUM_G, _COLSUM_V = "+k_colsum_partial<false>+k_colsum_final", "+k_colsum_partial<true>+k_colsum_final"
_TAIL_G = "+k_zero_rows+" + _GENERIC + "+k_scatter_mean"
_TAIL_V = "+k_zero_rows+k_gemm<64, 64, 2, 2, 1, 2>+k_scatter_mean"

# odd widths: the generic (scalar) kernel variants on the twin path, no statistics hand-off
_register(ModelCase("M1", SMALL_GRAPH, 100, 64, (5, 3), 37, 30, 3, 5, ((249, 588), (64, 249)),
                    forward=(("k_gemm<64, 64>", "k_gemm<64, 64>"), ("k_gemm<64, 64>", "k_gemm<64, 64>")),
                    backward=((_GENERIC + _COLSUM_G, _GENERIC + "[splits=2]+k_slab_reduce" + _COLSUM_G),
                              (_GENERIC + _COLSUM_G + _TAIL_G, _GENERIC + _COLSUM_G + _TAIL_G)),
                    bn_calls=(False,)))
# three hops: the middle layer has both extents and takes an input gradient that came through another layer (k_gemm_dual)
_register(ModelCase("M2", SMALL_GRAPH, 100, 128, (6, 4, 3), 40, 48, 4, 5, ((1209, 2059), (511, 1209), (128, 511)),
                    forward=(("k_gemm<64, 64>",) * 2,) * 3,
                    backward=((_VEC + "[splits=5]+k_slab_reduce" + _COLSUM_V, _VEC + "[splits=18]+k_slab_reduce" + _COLSUM_V),
                              (DUAL % 2, DUAL % 4),
                              (_VEC + _COLSUM_V + _TAIL_V, _VEC + _COLSUM_V + _TAIL_V)),
                    bn_calls=(False, False)))
# hand-off: 5 800 destinations is the smallest count among the forward shapes the suite uses at 256 -> 256 (4 096, 4 160, 5 800, 11 000) at
# which sage_conv_forward_indexed_stats reports statistics -- 4 096 and 4 160 take stream-K, which produces none; the batch (859 seeds from
# node 6 979 on) was searched so that the outer block has exactly that many.  Its backward is a stream-K weight gradient, the inner block
# (859 rows) takes k_gemm_dual + k_scatter_and_finals.
_register(ModelCase("M3", BIG_GRAPH, 6979, 859, (10, 8), 256, 256, 3, 5, ((5800, 19091), (859, 5800)),
                    forward=(("k_gather_beside_gemm<3>+k_gemm_tile16<3, 4>", "k_gather_beside_gemm<5>+k_gemm_tile16<5, 4>"),
                             ("k_gemm_tile16<1, 4>", "k_gemm_tile16<1, 4>")),
                    backward=((STREAMK_TN, STREAMK_TN), (DUAL % 4, DUAL % 4)),
                    bn_calls=(True,)))


def capacities(case: ModelCase):
    """(n_dst, n_src) capacities per block, outer -> inner, of a DeviceBatch of the case's shape."""
    t, out = case.batch, []
    for f in case.sizes:
        out.append((t, t + t * f))
        t = t + t * f
    return tuple(out[::-1])


def planned_names(lib, case: ModelCase, extent: bool, cus: int = CUS):
    """[(forward, backward)] per block as the library's plan functions print them for the shapes of the host-sized batch / the
    capacities: the first block runs behind IndexedFeatures (its backward sees the destination rows only and no input gradient), a
    hidden block whose forward hands statistics over takes its bias gradient from the BatchNorm backward."""
    import ctypes
    from graphpope_amd import _lib
    dims = capacities(case) if extent else case.host_dims
    out = []
    for i, (n_dst, n_src) in enumerate(dims):
        c_in = case.c_in if i == 0 else case.hidden
        f, b = ctypes.create_string_buffer(96), ctypes.create_string_buffer(256)
        _lib.check(lib.sage_forward_kernel_name(n_dst, c_in, case.hidden, cus, f, 96))
        handoff = i < len(dims) - 1 and f.value.decode().split("<")[0] in ("k_gemm_tile16", "k_gather_beside_gemm")
        _lib.check(lib.sage_backward_kernel_name(n_dst, n_dst if i == 0 else n_src, c_in, case.hidden, int(i > 0), int(not handoff), cus, b, 256))
        out.append((f.value.decode(), b.value.decode()))
    return out


def expected_names(case: ModelCase, extent: bool):
    return [(f[int(extent)], b[int(extent)]) for f, b in zip(case.forward, case.backward)]


@functools.lru_cache(maxsize=2)
def host_graph(graph):
    """(rowptr, col) int64 of the graph's CSR, as engine.build_csr lays it out from synth's sorted edge list."""
    from graphpope_amd import synth
    n, pairs, seed, alpha, shift = graph
    ei = synth.powerlaw_graph(n, pairs, seed=seed, alpha=alpha, shift=shift)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=n))]).astype(np.int64)
    return rowptr, np.asarray(ei[1], dtype=np.int64)


def case_seeds(case: ModelCase) -> np.ndarray:
    return np.arange(case.first_seed, case.first_seed + case.batch, dtype=np.int64)


@functools.lru_cache(maxsize=4)
def host_batch(case: ModelCase):
    """(n_id, blocks outer -> inner) of the case's batch from the CPU restatement of the sampler (oracle.sample_hop, pinned bit for bit
    to the kernels by tests/test_sampler_gpu.py).  A block is (rowptr, col, n_src) with int64 arrays."""
    from oracle import oracle
    rowptr, col = host_graph(case.graph)
    n_id, blocks = case_seeds(case), []
    for hop, size in enumerate(case.sizes):
        rp, cl, n_id = oracle.sample_hop(rowptr, col, n_id, size, case.sample_seed, hop)
        blocks.append((rp.astype(np.int64), cl.astype(np.int64), len(n_id)))
    return n_id, blocks[::-1]


def case_features(case: ModelCase) -> torch.Tensor:
    """float32 [N, c_in] on the CPU."""
    return torch.randn(case.graph[0], case.c_in, generator=torch.Generator().manual_seed(case.c_in + case.batch))


def case_labels(case: ModelCase) -> torch.Tensor:
    return torch.randint(0, CLASSES, (case.batch,), generator=torch.Generator().manual_seed(case.batch))


def host_inputs(case: ModelCase, seeds, seed_dev: int = 0) -> "Inputs":
    """The case on the CPU alone: the restated sampler's batch, the model's initial parameters, the given dropout seeds."""
    n_id, blocks = host_batch(case)
    state = {k: v.clone() for k, v in case_model(case).state_dict().items()}
    return Inputs(state, case_features(case)[torch.from_numpy(n_id)], list(blocks), case_labels(case), list(seeds), seed_dev)


def case_model(case: ModelCase):
    """graphpope_amd.sage.SAGE on the CPU with fixed parameters; BatchNorm's weights, biases and running statistics are moved off their
    defaults so that a swapped or skipped one shows."""
    from graphpope_amd.sage import SAGE
    torch.manual_seed(case.hidden * 1000 + case.c_in)
    model = SAGE(case.c_in, CLASSES, case.hidden, case.num_layers, dropout=P)
    with torch.no_grad():
        for b in model.bns:
            b.weight.uniform_(0.5, 1.5)
            b.bias.uniform_(-0.3, 0.3)
            b.running_mean.uniform_(-1, 1)
            b.running_var.uniform_(0.5, 2)
    return model


# ------------------------------------------------------------------------------------------------ the reference

class _Gate(torch.autograd.Function):
    """z * on * scale forward; backward with another (on, scale): only the mutants differ between the two."""

    @staticmethod
    def forward(ctx, z, on_f, s_f, on_b, s_b):
        ctx.save_for_backward(on_b)
        ctx.s_b = s_b
        return z * on_f * s_f

    @staticmethod
    def backward(ctx, g):
        on_b, = ctx.saved_tensors
        return g * on_b * ctx.s_b, None, None, None, None


class _ShiftGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return torch.roll(g, 1, 0)


@dataclass
class Inputs:
    """What one forward + backward pass of the model is a function of.  `state`: the model's state_dict as float32 CPU tensors; `x`: the
    feature rows of the batch's nodes, float32 [n_src of block 0, c_in]; `blocks`: (rowptr, col, n_src) outer -> inner at the true sizes;
    `seeds`: the dropout seed of every hidden layer; `seed_dev`: the device word added to them (0: none)."""
    state: dict
    x: torch.Tensor
    blocks: list
    y: torch.Tensor
    seeds: list
    seed_dev: int = 0
    p: float = P

    @property
    def hidden_layers(self):
        return len(self.blocks) - 1

    @functools.cached_property
    def keeps(self):
        return [torch.from_numpy(bn.keep_mask(self.seeds[i], len(self.blocks[i][0]) - 1, self.state["bns.%d.weight" % i].numel(), self.p,
                                              self.seed_dev)) for i in range(self.hidden_layers)]


@dataclass
class Run:
    out: dict                                      # name -> tensor (CPU): logits, loss, y.i, running_mean.i, running_var.i, grad:<parameter>
    z: list                                        # per hidden layer, detached
    patterns: list                                 # bool per hidden layer: the ReLU pattern used
    grad_h_abs: dict = field(default_factory=dict)  # bias name -> max_c sum_r |grad_h[r, c]|


def _edge_perm(nnz, k):
    return None if k == 0 else torch.from_numpy(np.random.RandomState(1000 + k).permutation(nnz))


def run_model(inp: Inputs, dtype, patterns=None, device_on=None, perm: int = 0, mutant: dict | None = None) -> Run:
    """SAGE.forward + F.cross_entropy + backward in `dtype`.

    patterns    None: z > 0.  A list of bool tensors: used as given (the restatement runs on the reference's pattern).
    device_on   list of bool tensors per hidden layer, y_device > 0: inside the gate (|z| < GATE) the pattern is the device's where the mask
                keeps the element.  Only with patterns=None.
    perm        0: edges in CSR order; k > 0: the k-th fixed permutation of every block's edge list.
    mutant      {"kind": ..., ...}: one thing wrong (test_sage_model_cpu.py); None: the model as it is."""
    mutant = mutant or {}
    kind = mutant.get("kind")
    st = {k: v.detach().to(dtype).requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in inp.state.items()
          if v.dtype.is_floating_point}
    h = inp.x.to(dtype)
    last = len(inp.blocks) - 1
    out, zs, pats, hs = {}, [], [], []
    ik = 1.0 / (1.0 - inp.p)
    for i, (rowptr, col, n_src) in enumerate(inp.blocks):
        assert h.shape[0] == n_src, (i, h.shape, n_src)
        n = len(rowptr) - 1
        deg = np.diff(rowptr)
        row, c = torch.from_numpy(np.repeat(np.arange(n), deg)), torch.from_numpy(np.asarray(col))
        if kind == "drop_edge" and i == last:
            assert deg[-1] > 0
            row, c = row[:-1], c[:-1]
        pm = _edge_perm(len(row), perm)
        if pm is not None:
            row, c = row[pm], c[pm]
        div = torch.from_numpy(np.maximum(deg, 1)).to(dtype)
        if kind == "deg_plus_one" and i == mutant["layer"]:
            div = div.clone()
            div[mutant["row"]] += 1
        if kind == "shift_grad_x" and i == last:
            h = _ShiftGrad.apply(h)
        agg = torch.zeros(n, h.shape[1], dtype=dtype).index_add_(0, row, h[c]) / div[:, None]
        w_l, b_l, w_r = st["convs.%d.lin_l.weight" % i], st["convs.%d.lin_l.bias" % i], st["convs.%d.lin_r.weight" % i]
        h = agg @ w_l.t() + b_l + h[:n] @ w_r.t()
        if i == last:
            break
        h.retain_grad()
        hs.append(h)
        gamma, beta = st["bns.%d.weight" % i], st["bns.%d.bias" % i]
        mu, var = h.mean(0), h.var(0, unbiased=False)
        z = (h - mu) / torch.sqrt(var + EPS) * gamma + beta
        zd = z.detach()
        if patterns is not None:
            pat = patterns[i]
        else:
            pat = zd > 0
            if device_on is not None:
                pat = torch.where((zd.abs() < GATE) & inp.keeps[i], device_on[i], pat)
        keep = inp.keeps[i]
        on = (pat & keep).to(dtype)
        if kind == "no_rescale_backward" and i == mutant["layer"]:
            h = _Gate.apply(z, on, ik, on, 1.0)
        elif kind == "backward_mask_seed" and i == mutant["layer"]:
            other = torch.from_numpy(bn.keep_mask(mutant["seed"], n, z.shape[1], inp.p, inp.seed_dev))
            h = _Gate.apply(z, on, ik, (pat & other).to(dtype), ik)
        else:
            h = z * on * ik
        h.retain_grad()
        with torch.no_grad():
            unbiased = var if kind == "biased_running_var" and i == mutant["layer"] else var * (n / (n - 1))
            out["running_mean.%d" % i] = (1 - MOMENTUM) * st["bns.%d.running_mean" % i] + MOMENTUM * mu
            out["running_var.%d" % i] = (1 - MOMENTUM) * st["bns.%d.running_var" % i] + MOMENTUM * unbiased
        out["y.%d" % i] = h
        zs.append(zd)
        pats.append(pat)
    loss = F.cross_entropy(h, inp.y)
    loss.backward()
    out["logits"], out["loss"] = h.detach(), loss.detach()
    for k, v in st.items():
        if v.grad is not None:
            out["grad:" + k] = v.grad
    run = Run(out, zs, pats)
    for i, hh in enumerate(hs):
        run.grad_h_abs["grad:convs.%d.lin_l.bias" % i] = float(hh.grad.abs().sum(0).max())
        if kind == "bias_from_grad_y" and i == mutant["layer"]:
            out["grad:convs.%d.lin_l.bias" % i] = out["y.%d" % i].grad.sum(0)
    for i in range(last):
        out["y.%d" % i] = out["y.%d" % i].detach()
    return run


# ------------------------------------------------------------------------------------------------ yardstick and check

@dataclass
class Yardstick:
    ref: Run
    scale: dict
    err32: dict
    gated: list                  # per hidden layer: gated elements
    elements: list
    mismatches: list             # per hidden layer: kept elements outside the gate whose device pattern differs from the reference's (None: no device)
    loss32: float


def _scales(ref: Run) -> dict:
    return {k: (ref.grad_h_abs[k] if k in ref.grad_h_abs else float(v.abs().max())) for k, v in ref.out.items() if k != "loss"}


def _errors(out: dict, ref: Run, scale: dict) -> dict:
    return {k: float((out[k].double() - ref.out[k]).abs().max()) / scale[k] for k in scale}


def yardstick(inp: Inputs, device_on=None) -> Yardstick:
    """The float64 reference (gate resolved with the device's pattern, if given) and the float32 restatement's errors against it."""
    ref = run_model(inp, torch.float64, device_on=device_on)
    gated = [int((z.abs() < GATE).sum()) for z in ref.z]
    elements = [z.numel() for z in ref.z]
    mismatches = None
    if device_on is not None:
        mismatches = [int((((z > 0) != d) & ~(z.abs() < GATE) & k).sum()) for z, d, k in zip(ref.z, device_on, inp.keeps)]
    scale = _scales(ref)
    err32, loss32 = {k: 0.0 for k in scale}, 0.0
    for k in range(PERMS):
        r = run_model(inp, torch.float32, patterns=ref.patterns, perm=k)
        for key, e in _errors(r.out, ref, scale).items():
            err32[key] = max(err32[key], e)
        loss32 = max(loss32, abs(float(r.out["loss"]) - float(ref.out["loss"])))
    return Yardstick(ref, scale, err32, gated, elements, mismatches, loss32)


def loss_bound(yard: Yardstick) -> float:
    s = yard.scale["logits"]
    return 2.0 * FACTOR * yard.err32["logits"] * s + 8.0 * 2.0 ** -24 * s


def check(yard: Yardstick, got: dict, name: str = "", must_hold: bool = True) -> dict:
    """`got`: name -> tensor as Run.out names them (hidden y at their true row counts).  Returns {"tensors": {name: {err_dev, err_32,
    ratio}}, "gated", "elements", "pattern_mismatches", "loss_err", "loss_bound", "worst"}; ratio = err_dev / (FACTOR * err_32) must be
    <= 1, the pattern outside the gate exact, the gate's share below the cap.  must_hold=False: report only (the mutants)."""
    rep = {"tensors": {}, "gated": yard.gated, "elements": yard.elements, "pattern_mismatches": yard.mismatches}
    assert set(got) >= set(yard.scale), (name, sorted(set(yard.scale) - set(got)))
    errs = _errors(got, yard.ref, yard.scale)
    worst = 0.0
    for k, e in errs.items():
        assert math.isfinite(e), (name, k, "non-finite")
        allowed = FACTOR * yard.err32[k]
        ratio = 0.0 if e == 0.0 else (e / allowed if allowed > 0 else math.inf)
        rep["tensors"][k] = {"err_dev": e, "err_32": yard.err32[k], "ratio": ratio}
        worst = max(worst, ratio)
    rep["loss_err"], rep["loss_bound"] = abs(float(got["loss"]) - float(yard.ref.out["loss"])), loss_bound(yard)
    rep["worst"] = max(worst, rep["loss_err"] / rep["loss_bound"])
    if must_hold:
        for g, m in zip(yard.gated, yard.elements):
            assert g <= bn.EXCLUDED_CAP * m, (name, "share of gated elements", g, m)
        assert yard.mismatches is None or not any(yard.mismatches), (name, "ReLU pattern differs outside the gate", yard.mismatches)
        bad = {k: v for k, v in rep["tensors"].items() if v["ratio"] > 1.0}
        assert not bad, (name, bad)
        assert rep["loss_err"] <= rep["loss_bound"], (name, "loss", rep["loss_err"], rep["loss_bound"])
    return rep


def device_patterns(got: dict, hidden_layers: int):
    return [got["y.%d" % i] > 0 for i in range(hidden_layers)]


# ------------------------------------------------------------------------------------------------ Adam

U = 2.0 ** -23


def adam_scalars(lr, beta1, beta2, eps, step):
    """(step_size, 1 - b1, b2, 1 - b2, eps, inv_bc2_sqrt) as float32: formed in double and rounded once, as the launcher and the kernel's
    device-step prologue form them."""
    bc1, bc2 = 1.0 - math.pow(beta1, float(step)), 1.0 - math.pow(beta2, float(step))
    f = np.float32
    return f(lr / bc1), f(1.0 - beta1), f(beta2), f(1.0 - beta2), f(eps), f(1.0 / math.sqrt(bc2))


def adam_reference(p, g, m, v, coef, lr, beta1, beta2, eps, step):
    """float64 Adam on float32 arrays (NumPy): (p', bound on |p_device - p'|) element-wise.  coef: the float32 clip coefficient the device
    reported (1 for none)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    bc1, bc2 = 1.0 - math.pow(beta1, float(step)), 1.0 - math.pow(beta2, float(step))
    ss, inv = lr / bc1, 1.0 / math.sqrt(bc2)
    gc = g * float(coef)
    mn = m + (gc - m) * (1.0 - beta1)
    vn = beta2 * v + (1.0 - beta2) * gc * gc
    root = np.sqrt(vn)
    d = root * inv + eps
    q = mn / d
    pn = p - ss * q
    omb1, omb2 = 1.0 - beta1, 1.0 - beta2
    dm = U * (omb1 * (np.abs(gc) + 3.0 * np.abs(gc - m)) + np.abs(mn))
    dv = U * (5.0 * omb2 * gc * gc + 2.0 * beta2 * v + vn) + 2.0 ** -126
    droot = np.sqrt(vn + dv) - np.sqrt(np.maximum(vn - dv, 0.0))
    dd = droot * inv + U * (3.0 * root * inv + eps + d)
    dq = dm / d + np.abs(q) * dd / d + U * np.abs(q)
    dp = ss * dq + 2.0 * U * ss * np.abs(q) + U * np.abs(pn)
    return pn, dp


def adam_restate32(p, g, m, v, coef, lr, beta1, beta2, eps, step):
    """k_adam's formula in NumPy float32, every operation rounded once: what a correct float32 implementation returns."""
    ss, omb1, b2, omb2, eps32, inv = adam_scalars(lr, beta1, beta2, eps, step)
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    gc = g * f(coef)
    mn = m + (gc - m) * omb1
    vn = b2 * v + omb2 * gc * gc
    pn = p - ss * (mn / (np.sqrt(vn) * inv + eps32))
    assert pn.dtype == f and mn.dtype == f and vn.dtype == f
    return pn, mn, vn


def expected_coef(norm32, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in IEEE float32."""
    c = np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else c
