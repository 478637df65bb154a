"""Cases, float64 references and thresholds for SAGEConv(normalize=True) and the models built from it (graphpope_amd/sage.py; PyG 1.7.0
SAGEConv: out = F.normalize(out, p=2., dim=-1) behind the two projections).  Imports without a GPU and is not a test module:
test_sage_normalize_cpu.py proves the references and the thresholds on the CPU, test_sage_normalize_gpu.py runs the kernels through them.

Conv (:func:`run_conv`): a dense formulation in plain torch under autograd, parameterised by dtype: the block as a dense [n_dst, n_src]
matrix of 1 / deg, out = normalize(A x W_l^T + b + x[:n_dst] W_r^T), loss = sum(out * G) for a fixed G, so the gradients of x, W_l, b and
W_r are those of an arbitrary upstream gradient.  In float64 it is the reference, in float32 the restatement.

Model (:func:`run_model`): sage_model_cases.run_model with the normalisation behind every conv -- per block the mean aggregation, the
projections, F.normalize, and on every block but the last batch statistics OF THE NORMALISED ROWS, the affine map, the ReLU pattern and
the restated dropout mask; then F.cross_entropy.  The gate of sage_model_cases.py applies unchanged (z is a BatchNorm output).
`wrong`: "shortcut_stats" takes the batch statistics from the un-normalised projection (what the projection's epilogue would hand over),
"shortcut_bias" takes the bias gradient of a hidden conv as the column sums of the gradient entering the normalisation's output (what the
BatchNorm backward pass would hand over).  Both must fall outside the threshold.

Error measure and threshold, the rule of sage_model_cases.py and full_inference_cases.py: err(T) = max |T - T_64| / max |T_64|,
err_dev(T) <= FACTOR * max(err_32(T), 2^-23) with err_32 the float32 restatement's error, the maximum over PERMS orders of the sums
(the model: permutations of every block's edge list; the conv: permutations of the source rows, which reorder the dense products), computed
from the reference side when the test runs.  FACTOR = 4: 2 for a second draw of the same rounding process, 2 for the kernels' different but
equally legitimate summation structure (MFMA tiles, split-K slabs, the wave fold of the normalisation).  The 2^-23 floor covers tensors
the restatement happens to hit exactly.  Unlike in sage_model_cases.py the bias gradient of a hidden conv is NOT zero in exact arithmetic
(the normalisation stands between the bias and BatchNorm), so it is measured like every other tensor.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import sage_model_cases as mc

FACTOR = mc.FACTOR
PERMS = mc.PERMS
FLOOR = 2.0 ** -23
L2_EPS = 1e-12

N_SRC, N_DST, C_IN = 70, 33, 12
C_OUTS = (5, 64)
EMPTY_ROW = 4
MANUAL_SEED = 77

# conv + BatchNorm at a shape whose plain projection hands its statistics to BatchNorm (k_gemm_tile16): the shortcut that a normalising
# conv must not take
HANDOFF = (2000, 2600, 64, 128)               # n_dst, n_src, c_in, c_out


# ------------------------------------------------------------------------------------------------ blocks

@functools.lru_cache(maxsize=None)
def block(n_dst: int, n_src: int, seed: int, max_deg: int = 6, empty_row: int | None = EMPTY_ROW):
    """(rowptr, col) int64 of a random bipartite block; destinations are the first n_dst sources.  Row `empty_row` has no neighbour."""
    rs = np.random.RandomState(seed)
    deg = rs.randint(1, max_deg + 1, size=n_dst)
    if empty_row is not None:
        deg[empty_row] = 0
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rs.randint(0, n_src, size=int(rowptr[-1])).astype(np.int64)
    return rowptr, col


def dense_mean(rowptr, col, n_src, dtype):
    n_dst = len(rowptr) - 1
    a = torch.zeros(n_dst, n_src, dtype=torch.float64)
    deg = np.diff(rowptr)
    rows = np.repeat(np.arange(n_dst), deg)
    a.index_put_((torch.from_numpy(rows), torch.from_numpy(np.asarray(col))), torch.ones(len(col), dtype=torch.float64), accumulate=True)
    return (a / torch.from_numpy(np.maximum(deg, 1)).to(torch.float64)[:, None]).to(dtype)


# ------------------------------------------------------------------------------------------------ one conv

@functools.lru_cache(maxsize=None)
def conv_inputs(c_out: int, bias: bool, shape=(N_DST, N_SRC, C_IN)):
    """name -> float32 CPU tensor: x, w_l, (b_l,) w_r and the upstream gradient g; plus the block."""
    n_dst, n_src, c_in = shape
    gen = torch.Generator().manual_seed(1000 * c_out + c_in + int(bias))
    bound = 1.0 / np.sqrt(c_in)
    t = {"x": torch.randn(n_src, c_in, generator=gen) + 0.25,
         "w_l": (torch.rand(c_out, c_in, generator=gen) * 2 - 1) * bound,
         "w_r": (torch.rand(c_out, c_in, generator=gen) * 2 - 1) * bound,
         "g": torch.randn(n_dst, c_out, generator=gen)}
    if bias:
        t["b_l"] = (torch.rand(c_out, generator=gen) * 2 - 1) * bound
    return t, block(n_dst, n_src, seed=c_out + n_dst)


def run_conv(t: dict, blk, dtype, normalize: bool = True, perm: int = 0) -> dict:
    """out and the gradients of x, w_l, (b_l,) w_r under loss = sum(out * g), on the CPU in `dtype`."""
    rowptr, col = blk
    n_dst, n_src = len(rowptr) - 1, t["x"].shape[0]
    leaf = {k: v.detach().to(dtype).requires_grad_(True) for k, v in t.items() if k != "g"}
    a, x = dense_mean(rowptr, col, n_src, dtype), leaf["x"]
    if perm:                                                  # another order of the sums over the sources
        p = torch.from_numpy(np.random.RandomState(300 + perm).permutation(n_src))
        agg = a[:, p] @ x[p]
    else:
        agg = a @ x
    out = agg @ leaf["w_l"].t() + x[:n_dst] @ leaf["w_r"].t()
    if "b_l" in leaf:
        out = out + leaf["b_l"]
    if normalize:
        out = F.normalize(out, p=2.0, dim=-1, eps=L2_EPS)
    (out * t["g"].to(dtype)).sum().backward()
    res = {"out": out.detach()}
    res.update({"grad:" + k: v.grad for k, v in leaf.items()})
    return res


def err(t, t64) -> float:
    t, t64 = torch.as_tensor(t).to(torch.float64), torch.as_tensor(t64).to(torch.float64)
    return float((t - t64).abs().max() / t64.abs().max())


def conv_yardstick(t: dict, blk, normalize: bool = True):
    """(reference, name -> threshold)."""
    ref = run_conv(t, blk, torch.float64, normalize)
    e32 = {k: 0.0 for k in ref}
    for perm in range(PERMS):
        r = run_conv(t, blk, torch.float32, normalize, perm)
        for k in ref:
            e32[k] = max(e32[k], err(r[k], ref[k]))
    return ref, {k: FACTOR * max(v, FLOOR) for k, v in e32.items()}


def conv_check(got: dict, ref: dict, limit: dict, name: str = "") -> float:
    """Prints every figure, then asserts; returns the worst err / limit."""
    assert set(got) == set(ref), (name, sorted(got), sorted(ref))
    worst = 0.0
    for k in sorted(ref):
        e = err(got[k], ref[k])
        print("%-28s %-14s err %.3e limit %.3e" % (name, k, e, limit[k]))
        worst = max(worst, e / limit[k])
    for k in sorted(ref):
        assert torch.isfinite(torch.as_tensor(got[k])).all() and err(got[k], ref[k]) <= limit[k], (name, k)
    return worst


# ------------------------------------------------------------------------------------------------ the two-layer model

MODEL = dict(c_in=12, classes=5, hidden=16, num_layers=2)
MODEL_DIMS = ((40, 90), (16, 40))             # (n_dst, n_src) outer -> inner


def model_blocks():
    out = []
    for i, (n_dst, n_src) in enumerate(MODEL_DIMS):
        rowptr, col = block(n_dst, n_src, seed=900 + i, empty_row=2)
        out.append((rowptr, col, n_src))
    return out


def build_model(p: float, normalize: bool = True, bias: bool = True):
    """graphpope_amd.sage.SAGE(12, 5, 16, 2, normalize=...) on the CPU with fixed parameters and BatchNorm moved off its defaults."""
    from graphpope_amd import sage
    torch.manual_seed(5)
    model = sage.SAGE(MODEL["c_in"], MODEL["classes"], MODEL["hidden"], MODEL["num_layers"], dropout=p, normalize=normalize)
    with torch.no_grad():
        for b in model.bns:
            b.weight.uniform_(0.5, 1.5)
            b.bias.uniform_(-0.3, 0.3)
            b.running_mean.uniform_(-1, 1)
            b.running_var.uniform_(0.5, 2)
    return model


def model_inputs(p: float, seeds) -> mc.Inputs:
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(MODEL_DIMS[0][1], MODEL["c_in"], generator=gen) + 0.25
    y = torch.randint(0, MODEL["classes"], (MODEL_DIMS[-1][0],), generator=gen)
    state = {k: v.clone() for k, v in build_model(p).state_dict().items()}
    return mc.Inputs(state, x, model_blocks(), y, list(seeds), 0, p)


def run_model(inp: mc.Inputs, dtype, patterns=None, device_on=None, perm: int = 0, wrong: str | None = None, normalize: bool = True) -> mc.Run:
    """SAGE.forward (training mode) + F.cross_entropy + backward in `dtype`; arguments as sage_model_cases.run_model."""
    st = {k: v.detach().to(dtype).requires_grad_("running" not in k) for k, v in inp.state.items() if v.dtype.is_floating_point}
    h = inp.x.to(dtype)
    last = len(inp.blocks) - 1
    out, zs, pats, normed = {}, [], [], []
    ik = 1.0 / (1.0 - inp.p)
    for i, (rowptr, col, n_src) in enumerate(inp.blocks):
        assert h.shape[0] == n_src
        n, deg = len(rowptr) - 1, np.diff(rowptr)
        row, c = torch.from_numpy(np.repeat(np.arange(n), deg)), torch.from_numpy(np.asarray(col))
        pm = mc._edge_perm(len(row), perm)
        if pm is not None:
            row, c = row[pm], c[pm]
        div = torch.from_numpy(np.maximum(deg, 1)).to(dtype)
        agg = torch.zeros(n, h.shape[1], dtype=dtype).index_add_(0, row, h[c]) / div[:, None]
        raw = agg @ st["convs.%d.lin_l.weight" % i].t() + h[:n] @ st["convs.%d.lin_r.weight" % i].t()
        if "convs.%d.lin_l.bias" % i in st:
            raw = raw + st["convs.%d.lin_l.bias" % i]
        h = F.normalize(raw, p=2.0, dim=-1, eps=L2_EPS) if normalize else raw
        if i == last:
            break
        h.retain_grad()
        normed.append(h)
        gamma, beta = st["bns.%d.weight" % i], st["bns.%d.bias" % i]
        stats_of = raw.detach() if wrong == "shortcut_stats" else h
        mu, var = stats_of.mean(0), stats_of.var(0, unbiased=False)
        z = (h - mu) / torch.sqrt(var + mc.EPS) * gamma + beta
        zd = z.detach()
        if patterns is not None:
            pat = patterns[i]
        else:
            pat = zd > 0
            if device_on is not None:
                pat = torch.where((zd.abs() < mc.GATE) & inp.keeps[i], device_on[i], pat)
        h = z * (pat & inp.keeps[i]).to(dtype) * ik
        with torch.no_grad():
            out["running_mean.%d" % i] = (1 - mc.MOMENTUM) * st["bns.%d.running_mean" % i] + mc.MOMENTUM * mu
            out["running_var.%d" % i] = (1 - mc.MOMENTUM) * st["bns.%d.running_var" % i] + mc.MOMENTUM * var * (n / (n - 1))
        out["y.%d" % i] = h.detach()
        zs.append(zd)
        pats.append(pat)
    loss = F.cross_entropy(h, inp.y)
    loss.backward()
    out["logits"], out["loss"] = h.detach(), loss.detach()
    for k, v in st.items():
        if v.grad is not None:
            out["grad:" + k] = v.grad
    if wrong == "shortcut_bias":
        for i, hh in enumerate(normed):
            out["grad:convs.%d.lin_l.bias" % i] = hh.grad.sum(0)
    return mc.Run(out, zs, pats)


def yardstick(inp: mc.Inputs, device_on=None) -> mc.Yardstick:
    """sage_model_cases.yardstick over :func:`run_model`, with the 2^-23 floor under every err_32."""
    ref = run_model(inp, torch.float64, device_on=device_on)
    gated = [int((z.abs() < mc.GATE).sum()) for z in ref.z]
    elements = [z.numel() for z in ref.z]
    mismatches = None
    if device_on is not None:
        mismatches = [int((((z > 0) != d) & ~(z.abs() < mc.GATE) & k).sum()) for z, d, k in zip(ref.z, device_on, inp.keeps)]
    scale = mc._scales(ref)
    err32, loss32 = {k: FLOOR for k in scale}, 0.0
    for k in range(PERMS):
        r = run_model(inp, torch.float32, patterns=ref.patterns, perm=k)
        for key, e in mc._errors(r.out, ref, scale).items():
            err32[key] = max(err32[key], e)
        loss32 = max(loss32, abs(float(r.out["loss"]) - float(ref.out["loss"])))
    return mc.Yardstick(ref, scale, err32, gated, elements, mismatches, loss32)


# ------------------------------------------------------------------------------------------------ conv + BatchNorm + ReLU as one node

def conv_bn_inputs():
    """HANDOFF's conv inputs plus gamma / beta and an upstream gradient for the BatchNorm output."""
    n_dst, n_src, c_in, c_out = HANDOFF
    t, blk = conv_inputs(c_out, True, (n_dst, n_src, c_in))
    gen = torch.Generator().manual_seed(8)
    t = dict(t, gamma=torch.rand(c_out, generator=gen) + 0.5, beta=torch.rand(c_out, generator=gen) * 0.6 - 0.3)
    return t, blk


def run_conv_bn(t: dict, blk, dtype, pattern=None, device_on=None, perm: int = 0, wrong: str | None = None):
    """y = relu(BatchNorm_train(normalize(conv(x)))) and the gradients of x, w_l, b_l, w_r, gamma, beta under loss = sum(y * g); also
    (z, pattern).  The ReLU pattern as in run_model: given, or z > 0 with the device's pattern inside the gate."""
    rowptr, col = blk
    n_dst, n_src = len(rowptr) - 1, t["x"].shape[0]
    leaf = {k: v.detach().to(dtype).requires_grad_(True) for k, v in t.items() if k != "g"}
    a, x = dense_mean(rowptr, col, n_src, dtype), leaf["x"]
    if perm:
        p = torch.from_numpy(np.random.RandomState(300 + perm).permutation(n_src))
        agg = a[:, p] @ x[p]
    else:
        agg = a @ x
    raw = agg @ leaf["w_l"].t() + x[:n_dst] @ leaf["w_r"].t() + leaf["b_l"]
    h = F.normalize(raw, p=2.0, dim=-1, eps=L2_EPS)
    h.retain_grad()
    stats_of = raw.detach() if wrong == "shortcut_stats" else h
    mu, var = stats_of.mean(0), stats_of.var(0, unbiased=False)
    z = (h - mu) / torch.sqrt(var + mc.EPS) * leaf["gamma"] + leaf["beta"]
    zd = z.detach()
    if pattern is None:
        pattern = zd > 0
        if device_on is not None:
            pattern = torch.where(zd.abs() < mc.GATE, device_on, pattern)
    y = z * pattern.to(dtype)
    (y * t["g"].to(dtype)).sum().backward()
    res = {"out": y.detach()}
    res.update({"grad:" + k: v.grad for k, v in leaf.items()})
    if wrong == "shortcut_bias":
        res["grad:b_l"] = h.grad.sum(0)
    return res, zd, pattern


def conv_bn_yardstick(t: dict, blk, device_on=None):
    """(reference, name -> threshold, gated elements, pattern mismatches outside the gate)."""
    ref, z, pattern = run_conv_bn(t, blk, torch.float64, device_on=device_on)
    e32 = {k: 0.0 for k in ref}
    for perm in range(PERMS):
        r, _, _ = run_conv_bn(t, blk, torch.float32, pattern=pattern, perm=perm)
        for k in ref:
            e32[k] = max(e32[k], err(r[k], ref[k]))
    gate = z.abs() < mc.GATE
    mismatches = 0 if device_on is None else int((((z > 0) != device_on) & ~gate).sum())
    return ref, {k: FACTOR * max(v, FLOOR) for k, v in e32.items()}, int(gate.sum()), mismatches


# ------------------------------------------------------------------------------------------------ evaluation over the whole graph

EVAL_N = 200


def eval_graph():
    return block(EVAL_N, EVAL_N, seed=41, max_deg=9, empty_row=2)


def eval_model(num_layers: int, normalize: bool = True):
    from graphpope_amd import sage
    torch.manual_seed(60 + num_layers)
    model = sage.SAGE(MODEL["c_in"], MODEL["classes"], MODEL["hidden"], num_layers, normalize=normalize)
    with torch.no_grad():
        for b in model.bns:
            b.weight.uniform_(0.5, 1.5)
            b.bias.uniform_(-0.3, 0.3)
            b.running_mean.uniform_(-0.2, 0.2)
            b.running_var.uniform_(0.01, 0.1)               # unit rows of 16 columns: entries of about 1/4
    return model


def eval_x():
    return torch.randn(EVAL_N, MODEL["c_in"], generator=torch.Generator().manual_seed(42)) + 0.25


def run_eval(state: dict, hops: int, dtype, perm: int = 0) -> torch.Tensor:
    """SAGE.forward in eval mode over `hops` copies of the whole graph, every conv normalising: conv, F.normalize, then on every hop
    but the last BatchNorm on the running statistics and ReLU."""
    rowptr, col = eval_graph()
    deg = np.diff(rowptr)
    row, c = torch.from_numpy(np.repeat(np.arange(EVAL_N), deg)), torch.from_numpy(col)
    pm = mc._edge_perm(len(row), perm)
    if pm is not None:
        row, c = row[pm], c[pm]
    div = torch.from_numpy(np.maximum(deg, 1)).to(dtype)
    h = eval_x().to(dtype)
    for i in range(hops):
        g = lambda k: state[k].to(dtype)
        agg = torch.zeros(EVAL_N, h.shape[1], dtype=dtype).index_add_(0, row, h[c]) / div[:, None]
        h = agg @ g("convs.%d.lin_l.weight" % i).t() + g("convs.%d.lin_l.bias" % i) + h @ g("convs.%d.lin_r.weight" % i).t()
        h = F.normalize(h, p=2.0, dim=-1, eps=L2_EPS)
        if i < hops - 1:
            h = ((h - g("bns.%d.running_mean" % i)) / torch.sqrt(g("bns.%d.running_var" % i) + mc.EPS) * g("bns.%d.weight" % i)
                 + g("bns.%d.bias" % i)).relu()
    return h


def eval_yardstick(state: dict, hops: int):
    ref = run_eval(state, hops, torch.float64)
    return ref, FACTOR * max(max(err(run_eval(state, hops, torch.float32, perm), ref) for perm in range(PERMS)), FLOOR)
