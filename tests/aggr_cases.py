"""Cases, restatements, float64 references and thresholds for SAGEConv(aggr='add' | 'max') (graphpope_amd/sage.py, csrc/aggregate.hip;
include/graphpope_hip.h, "Sum and max aggregation", is the contract).  Imports without a GPU and is not a test module:
test_aggr_cpu.py proves the restatement and the references on the CPU, test_aggr_gpu.py holds the two kernels to the restatement bit for
bit, test_sage_aggr_gpu.py runs the layer and the models through the float64 references.

Restatement (:func:`gather_restate`, :func:`scatter_restate`): the contract as sequential NumPy float32 loops -- one accumulator per
column, slots in ascending order, no fused operation (there is no product in either half).  The kernels must return its bits.

Float64 conv (:func:`run_conv`) and two-layer model (:func:`run_model`): the gather formulation in plain torch under autograd.  add:
index_add_ over the edge list.  max: arg by the first-slot rule (gather_restate on the values at hand), then agg = h[arg, column], so
autograd routes the gradient through the gathered entries -- once per (row, column), to the recorded source.  In float64 they are the
reference, in float32 the restatement whose error is the yardstick.

Error measure and threshold, the project's rule (sage_model_cases.py, sage_normalize_cases.py): err(T) = max |T - T_64| / max |T_64|,
err_dev(T) <= FACTOR * max(err_32(T), 2^-23), err_32 the maximum over PERMS float32 restatements computed when the test runs.  For add
the restatements permute the neighbour order (the edge list) and the c_in order of the products; for max only the c_in order, because a
permutation of the neighbours moves ties legitimately (the first of two equal values wins).

The max gate (the model): a float32 hidden activation within rounding of another may hand the maximum to either source, and one such
swap moves a whole gradient term.  An element (row, column) of a block whose input is a computed activation is gated when the reference's
best value and its best value from a DIFFERENT source lie within GATE * max |y| of each other -- except when both are exact zeros: those are
entries the ReLU or the dropout mask switched off, the same entries on the device (the ReLU gate of sage_model_cases.py holds the device
to that pattern), so the tie is a tie on both sides and the first-slot rule settles it the same way.  A gated element takes the device's arg
(restated from the device's own hidden activations: test_aggr_gpu.py holds the kernel to that restatement); elsewhere the device's arg
must equal the reference's.  The gated share is at most bn_epilogue_cases.EXCLUDED_CAP; the inner block of the model has 256 elements, so
the seeds are chosen for a reference without any gated element (asserted in test_aggr_cpu.py).  The first block aggregates the input
features, equal on both sides: no gate there.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import bn_epilogue_cases as bn
import sage_model_cases as mc
import sage_normalize_cases as sn

FACTOR, PERMS, FLOOR, GATE = mc.FACTOR, mc.PERMS, 2.0 ** -23, mc.GATE
AGGRS = ("add", "max")
AGGR_ID = {"mean": 0, "add": 1, "max": 2}

N_SRC, N_DST, C_IN, C_OUTS = sn.N_SRC, sn.N_DST, sn.C_IN, sn.C_OUTS
HANDOFF = sn.HANDOFF
MANUAL_SEED = 77
MODEL_P = 0.5


# ------------------------------------------------------------------------------------------------ the restatement

def gather_restate(rowptr, col, x, aggr, n_id=None):
    """(agg, arg) of the forward contract: x [rows, c] (float32 for the restatement; any float dtype), the block as int arrays; n_id:
    source j lives in row n_id[j].  arg int32 [n_dst, c] under max (block-local ids, -1 for an empty row), None under add.
    Step k folds slot k of every row that has one: each row still sees its own slots one by one, in ascending order."""
    x, rowptr, col = np.asarray(x), np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n_dst, c = len(rowptr) - 1, x.shape[1]
    deg = np.diff(rowptr)
    agg = np.zeros((n_dst, c), dtype=x.dtype)                        # +0.0: what an empty row keeps
    arg = np.full((n_dst, c), -1, dtype=np.int32) if aggr == "max" else None
    for k in range(int(deg.max()) if n_dst else 0):
        rows = np.nonzero(deg > k)[0]
        j = col[rowptr[rows] + k]
        v = x[j if n_id is None else np.asarray(n_id)[j]]
        if aggr == "add":
            agg[rows] = agg[rows] + v
        elif k == 0:                                                 # best starts from the first slot, never from 0
            agg[rows], arg[rows] = v, j[:, None].astype(np.int32)
        else:
            best = agg[rows]
            with np.errstate(invalid="ignore"):
                take = (v > best) | (np.isnan(v) & ~np.isnan(best))
            agg[rows] = np.where(take, v, best)
            arg[rows] = np.where(take, j[:, None].astype(np.int32), arg[rows])
    return agg, arg


def scatter_restate(rowptr, col, n_src, n_dst, grad_agg, grad_x, aggr, arg=None):
    """The backward contract: the grad_x [>= n_src, c] found on entry -> the one left behind (rows at or beyond n_src keep what they held).
    Step r adds the r-th slot (in ascending order) of every source that has one: each source still sees its own slots one by one."""
    grad_agg, out = np.asarray(grad_agg, dtype=np.float32), np.array(grad_x, dtype=np.float32, copy=True)
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    out[n_dst:n_src] = 0.0
    nnz = int(rowptr[n_dst])
    row = np.repeat(np.arange(n_dst), np.diff(rowptr[:n_dst + 1]))
    slots = np.nonzero((col[:nnz] >= 0) & (col[:nnz] < n_src))[0]    # out-of-range sources are skipped
    if aggr == "max":                                                # ... and so is every slot but the FIRST of its row that names its source
        _, first = np.unique(row[slots] * np.int64(n_src) + col[slots], return_index=True)
        slots = slots[np.sort(first)]
    order = slots[np.argsort(col[slots], kind="stable")]             # by source, ascending slot inside a source
    j = col[order]
    rank = np.arange(len(j)) - np.searchsorted(j, j, side="left")    # the slot's place among its source's slots
    for r in range(int(rank.max()) + 1 if len(j) else 0):
        at = order[rank == r]
        jj, ii = col[at], row[at]
        if aggr == "add":
            out[jj] = out[jj] + grad_agg[ii]
        else:                                                        # only in the columns the source won; elsewhere nothing is added, not +0
            m = arg[ii] == jj[:, None]
            out[jj] = np.where(m, out[jj] + grad_agg[ii], out[jj])
    return out


# ------------------------------------------------------------------------------------------------ blocks and values for the two halves

def degree_block(n_src: int, seed: int = 0, extra_dst: int = 0):
    """(rowptr, col) int32: rows of degree 0, 1 .. 9 (every remainder of the four-in-flight loop, twice over), one of 70 (past a 64-lane
    chunk), one that names a source three times and another twice, then `extra_dst` rows of degree 1 .. 6.  Sources are drawn from
    [0, n_src - 3): the last three sources are listed by nobody."""
    rs = np.random.RandomState(seed)
    rows = [rs.randint(0, n_src - 3, size=d) for d in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 70)]
    rows.append(np.array([5, 2, 5, 9, 5, 2]))
    rows += [rs.randint(0, n_src - 3, size=rs.randint(1, 7)) for _ in range(extra_dst)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rowptr, np.concatenate(rows).astype(np.int32)


def hub_block(n_src: int, n_dst: int = 130, hub: int = 3, seed: int = 1):
    """130 destinations that all name source `hub` (its list is longer than a wave), some of them twice, each beside 0 .. 3 others."""
    rs = np.random.RandomState(seed)
    rows = []
    for i in range(n_dst):
        others = rs.randint(0, n_src, size=i % 4)
        rows.append(rs.permutation(np.concatenate([others, [hub] * (2 if i % 7 == 0 else 1)])))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rowptr, np.concatenate(rows).astype(np.int32)


def half_values(rows: int, c: int, seed: int, nan_at=None):
    """float32 [rows, c]: column 0 negative throughout, 60 % exact zeros elsewhere (ties), optionally one NaN."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((rows, c)).astype(np.float32)
    x[rs.random_sample((rows, c)) < 0.6] = 0.0
    x[:, 0] = -np.abs(rs.standard_normal(rows).astype(np.float32)) - 0.5
    if nan_at is not None:
        x[nan_at] = np.nan
    return x


# ------------------------------------------------------------------------------------------------ one conv

def _depth_perm(c_in: int, perm: int):
    return None if perm == 0 else torch.from_numpy(np.random.RandomState(500 + perm).permutation(c_in))


def _aggregate(h, rowptr, col, aggr, dtype, edge_perm=None):
    """torch, under autograd: (agg, arg) of `h` over the block.  edge_perm: another order of the additions (add only)."""
    n, deg = len(rowptr) - 1, np.diff(rowptr)
    if aggr == "add":
        row, c = torch.from_numpy(np.repeat(np.arange(n), deg)), torch.from_numpy(np.asarray(col, dtype=np.int64))
        if edge_perm is not None:
            row, c = row[edge_perm], c[edge_perm]
        return torch.zeros(n, h.shape[1], dtype=dtype).index_add_(0, row, h[c]), None
    _, arg = gather_restate(rowptr, col, h.detach().numpy(), "max")
    a = torch.from_numpy(arg.astype(np.int64))
    picked = h[a.clamp(min=0), torch.arange(h.shape[1])[None, :].expand_as(a)]
    return torch.where(a >= 0, picked, torch.zeros((), dtype=dtype)), arg


def run_conv(t: dict, blk, dtype, aggr: str, perm: int = 0) -> dict:
    """out and the gradients of x, w_l, (b_l,) w_r under loss = sum(out * g), on the CPU in `dtype`; perm > 0: another order of the
    sums (module docstring)."""
    rowptr, col = blk
    n_dst = len(rowptr) - 1
    leaf = {k: v.detach().to(dtype).requires_grad_(True) for k, v in t.items() if k not in ("g", "gamma", "beta")}
    x = leaf["x"]
    agg, arg = _aggregate(x, rowptr, col, aggr, dtype, mc._edge_perm(len(col), perm) if aggr == "add" else None)
    dp = _depth_perm(x.shape[1], perm)
    if dp is None:
        out = agg @ leaf["w_l"].t() + x[:n_dst] @ leaf["w_r"].t()
    else:
        out = agg[:, dp] @ leaf["w_l"][:, dp].t() + x[:n_dst][:, dp] @ leaf["w_r"][:, dp].t()
    if "b_l" in leaf:
        out = out + leaf["b_l"]
    (out * t["g"].to(dtype)).sum().backward()
    res = {"out": out.detach()}
    res.update({"grad:" + k: v.grad for k, v in leaf.items()})
    return res


err = sn.err
conv_check = sn.conv_check
conv_inputs = sn.conv_inputs


def conv_yardstick(t: dict, blk, aggr: str):
    """(reference, name -> threshold)."""
    ref = run_conv(t, blk, torch.float64, aggr)
    e32 = {k: 0.0 for k in ref}
    for perm in range(PERMS):
        r = run_conv(t, blk, torch.float32, aggr, perm)
        for k in ref:
            e32[k] = max(e32[k], err(r[k], ref[k]))
    return ref, {k: FACTOR * max(v, FLOOR) for k, v in e32.items()}


# ------------------------------------------------------------------------------------------------ conv + BatchNorm + ReLU as one node

def run_conv_bn(t: dict, blk, dtype, aggr: str, pattern=None, device_on=None, perm: int = 0):
    """y = relu(BatchNorm_train(conv(x))) and the gradients of x, w_l, b_l, w_r, gamma, beta under loss = sum(y * g); also (z, pattern).
    The ReLU pattern as in sage_normalize_cases.run_conv_bn: given, or z > 0 with the device's pattern inside the gate."""
    rowptr, col = blk
    n_dst = len(rowptr) - 1
    leaf = {k: v.detach().to(dtype).requires_grad_(True) for k, v in t.items() if k != "g"}
    x = leaf["x"]
    agg, _ = _aggregate(x, rowptr, col, aggr, dtype, mc._edge_perm(len(col), perm) if aggr == "add" else None)
    dp = _depth_perm(x.shape[1], perm)
    if dp is None:
        h = agg @ leaf["w_l"].t() + x[:n_dst] @ leaf["w_r"].t() + leaf["b_l"]
    else:
        h = agg[:, dp] @ leaf["w_l"][:, dp].t() + x[:n_dst][:, dp] @ leaf["w_r"][:, dp].t() + leaf["b_l"]
    h.retain_grad()
    mu, var = h.mean(0), h.var(0, unbiased=False)
    z = (h - mu) / torch.sqrt(var + mc.EPS) * leaf["gamma"] + leaf["beta"]
    zd = z.detach()
    if pattern is None:
        pattern = zd > 0
        if device_on is not None:
            pattern = torch.where(zd.abs() < GATE, device_on, pattern)
    y = z * pattern.to(dtype)
    (y * t["g"].to(dtype)).sum().backward()
    res = {"out": y.detach()}
    res.update({"grad:" + k: v.grad for k, v in leaf.items()})
    return res, zd, pattern, float(h.grad.abs().sum(0).max())


def conv_bn_yardstick(t: dict, blk, aggr: str, device_on=None):
    """(reference, name -> threshold, gated elements, pattern mismatches outside the gate).  The bias gradient of a conv in front of a
    training-mode BatchNorm is zero in exact arithmetic: it is measured against the sum whose cancellation produces it, as in
    sage_model_cases.py, by scaling both sides (returned as the entry "scale:b_l")."""
    ref, z, pattern, b_scale = run_conv_bn(t, blk, torch.float64, aggr, device_on=device_on)
    e32 = {k: 0.0 for k in ref}
    for perm in range(PERMS):
        r, _, _, _ = run_conv_bn(t, blk, torch.float32, aggr, pattern=pattern, perm=perm)
        for k in ref:
            e = float((r[k].double() - ref[k]).abs().max()) / b_scale if k == "grad:b_l" else err(r[k], ref[k])
            e32[k] = max(e32[k], e)
    gate = z.abs() < GATE
    mismatches = 0 if device_on is None else int((((z > 0) != device_on) & ~gate).sum())
    limit = {k: FACTOR * max(v, FLOOR) for k, v in e32.items()}
    return ref, limit, int(gate.sum()), mismatches, b_scale


def conv_bn_check(got: dict, ref: dict, limit: dict, b_scale: float, name: str = ""):
    """conv_check with the bias gradient on its own scale."""
    assert set(got) == set(ref), (name, sorted(got), sorted(ref))
    errs = {k: (float((got[k].double() - ref[k]).abs().max()) / b_scale if k == "grad:b_l" else err(got[k], ref[k])) for k in ref}
    for k in sorted(ref):
        print("%-28s %-14s err %.3e limit %.3e" % (name, k, errs[k], limit[k]))
    for k in sorted(ref):
        assert torch.isfinite(got[k]).all() and errs[k] <= limit[k], (name, k, errs[k], limit[k])


# ------------------------------------------------------------------------------------------------ the two-layer model

MODEL, MODEL_DIMS = sn.MODEL, sn.MODEL_DIMS


def build_model(aggr: str, p: float = MODEL_P):
    """graphpope_amd.sage.SAGE(12, 5, 16, 2, aggr=...) on the CPU: sage_normalize_cases.build_model's parameters (the state dict does not
    depend on the aggregator)."""
    from graphpope_amd import sage
    torch.manual_seed(5)
    model = sage.SAGE(MODEL["c_in"], MODEL["classes"], MODEL["hidden"], MODEL["num_layers"], dropout=p, aggr=aggr)
    with torch.no_grad():
        for b in model.bns:
            b.weight.uniform_(0.5, 1.5)
            b.bias.uniform_(-0.3, 0.3)
            b.running_mean.uniform_(-1, 1)
            b.running_var.uniform_(0.5, 2)
    return model


def model_inputs(seeds, p: float = MODEL_P) -> mc.Inputs:
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(MODEL_DIMS[0][1], MODEL["c_in"], generator=gen) + 0.25
    y = torch.randint(0, MODEL["classes"], (MODEL_DIMS[-1][0],), generator=gen)
    state = {k: v.clone() for k, v in build_model("add", p).state_dict().items()}
    return mc.Inputs(state, x, sn.model_blocks(), y, list(seeds), 0, p)


def near_ties(h, rowptr, col, arg):
    """bool [n_dst, c]: the elements the max gate covers (module docstring) for the float64 activations `h` and their arg."""
    h = np.asarray(h, dtype=np.float64)
    scale = GATE * float(np.abs(h).max())
    gated = np.zeros(arg.shape, dtype=bool)
    for i in range(len(rowptr) - 1):
        beg, end = int(rowptr[i]), int(rowptr[i + 1])
        if end == beg:
            continue
        best = h[np.maximum(arg[i], 0), np.arange(h.shape[1])]
        for p in range(beg, end):
            j = int(col[p])
            other = arg[i] != j
            v = h[j]
            gated[i] |= other & (best - v < scale) & ~((best == 0.0) & (v == 0.0))
    return gated


def run_model(inp: mc.Inputs, dtype, aggr: str, patterns=None, device_on=None, device_arg=None, perm: int = 0):
    """SAGE.forward (training mode) + F.cross_entropy + backward in `dtype`: sage_model_cases.run_model with the aggregator in the mean's
    place.  Returns (mc.Run, args, ties): per block the arg used (None under add) and the gated elements of the max gate (None for the
    first block and under add).  device_arg: per block, the device's arg -- taken inside the gate."""
    st = {k: v.detach().to(dtype).requires_grad_("running" not in k) for k, v in inp.state.items() if v.dtype.is_floating_point}
    h = inp.x.to(dtype)
    last = len(inp.blocks) - 1
    out, zs, pats, hs, args, ties = {}, [], [], [], [], []
    ik = 1.0 / (1.0 - inp.p)
    for i, (rowptr, col, n_src) in enumerate(inp.blocks):
        assert h.shape[0] == n_src
        n = len(rowptr) - 1
        agg, arg = _aggregate(h, rowptr, col, aggr, dtype, mc._edge_perm(len(col), perm) if aggr == "add" else None)
        tie = None
        if aggr == "max" and i > 0:
            tie = near_ties(h.detach().numpy(), rowptr, col, arg)
            if device_arg is not None and tie.any():                 # inside the gate: the derivative of the function the device computed
                arg = np.where(tie, device_arg[i], arg)
                a = torch.from_numpy(arg.astype(np.int64))
                agg = torch.where(a >= 0, h[a.clamp(min=0), torch.arange(h.shape[1])[None, :].expand_as(a)], torch.zeros((), dtype=dtype))
        args.append(arg)
        ties.append(tie)
        w_l, b_l, w_r = st["convs.%d.lin_l.weight" % i], st["convs.%d.lin_l.bias" % i], st["convs.%d.lin_r.weight" % i]
        dp = _depth_perm(h.shape[1], perm)
        if dp is None:
            h = agg @ w_l.t() + b_l + h[:n] @ w_r.t()
        else:
            h = agg[:, dp] @ w_l[:, dp].t() + b_l + h[:n][:, dp] @ w_r[:, dp].t()
        if i == last:
            break
        h.retain_grad()
        hs.append(h)
        gamma, beta = st["bns.%d.weight" % i], st["bns.%d.bias" % i]
        mu, var = h.mean(0), h.var(0, unbiased=False)
        z = (h - mu) / torch.sqrt(var + mc.EPS) * gamma + beta
        zd = z.detach()
        if patterns is not None:
            pat = patterns[i]
        else:
            pat = zd > 0
            if device_on is not None:
                pat = torch.where((zd.abs() < GATE) & inp.keeps[i], device_on[i], pat)
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
    run = mc.Run(out, zs, pats)
    for i, hh in enumerate(hs):
        run.grad_h_abs["grad:convs.%d.lin_l.bias" % i] = float(hh.grad.abs().sum(0).max())
    return run, args, ties


def yardstick(inp: mc.Inputs, aggr: str, device_on=None, device_arg=None):
    """(mc.Yardstick, args, ties) over :func:`run_model`, with the 2^-23 floor under every err_32.  The float32 restatements run on the
    reference's ReLU pattern; under max their arg is their own (only the c_in order is permuted, so it moves only inside the gate)."""
    ref, args, ties = run_model(inp, torch.float64, aggr, device_on=device_on, device_arg=device_arg)
    gated = [int((z.abs() < GATE).sum()) for z in ref.z]
    elements = [z.numel() for z in ref.z]
    mismatches = None
    if device_on is not None:
        mismatches = [int((((z > 0) != d) & ~(z.abs() < GATE) & k).sum()) for z, d, k in zip(ref.z, device_on, inp.keeps)]
    scale = mc._scales(ref)
    err32, loss32 = {k: FLOOR for k in scale}, 0.0
    for k in range(PERMS):
        r, _, _ = run_model(inp, torch.float32, aggr, patterns=ref.patterns, device_arg=args if aggr == "max" else None, perm=k)
        for key, e in mc._errors(r.out, ref, scale).items():
            err32[key] = max(err32[key], e)
        loss32 = max(loss32, abs(float(r.out["loss"]) - float(ref.out["loss"])))
    return mc.Yardstick(ref, scale, err32, gated, elements, mismatches, loss32), args, ties


def arg_gate_check(args, ties, device_arg, name: str = ""):
    """The max gate's two assertions for every block behind the first: the share of gated elements, and the device's arg outside it."""
    for i, (arg, tie) in enumerate(zip(args, ties)):
        if tie is None:
            continue
        share, differ = float(tie.mean()), int(((arg != device_arg[i]) & ~tie).sum())
        print("%s block %d: %d of %d elements inside the max gate, %d args differ outside it" % (name, i, int(tie.sum()), tie.size, differ))
        assert share <= bn.EXCLUDED_CAP, (name, i, "share of gated elements", share)
        assert differ == 0, (name, i, "arg differs outside the gate", differ)


@functools.lru_cache(maxsize=None)
def model_seeds():
    """The dropout seeds SAGE.forward draws after torch.manual_seed(MANUAL_SEED)."""
    return tuple(mc.drawn_seeds(MANUAL_SEED, 1))


# ------------------------------------------------------------------------------------------------ evaluation over the whole graph

EVAL_N = sn.EVAL_N
eval_graph, eval_x = sn.eval_graph, sn.eval_x


def eval_model(num_layers: int, aggr: str):
    from graphpope_amd import sage
    torch.manual_seed(60 + num_layers)
    model = sage.SAGE(MODEL["c_in"], MODEL["classes"], MODEL["hidden"], num_layers, aggr=aggr)
    with torch.no_grad():
        for b in model.bns:
            b.weight.uniform_(0.5, 1.5)
            b.bias.uniform_(-0.3, 0.3)
            b.running_mean.uniform_(-1, 1)
            b.running_var.uniform_(0.5, 2)
    return model


def run_eval(state: dict, hops: int, dtype, aggr: str, perm: int = 0) -> torch.Tensor:
    """SAGE.forward in eval mode over `hops` copies of the whole graph: conv, then on every hop but the last BatchNorm on the running
    statistics and ReLU."""
    rowptr, col = eval_graph()
    h = eval_x().to(dtype)
    for i in range(hops):
        g = lambda k: state[k].to(dtype)
        agg, _ = _aggregate(h, rowptr, col, aggr, dtype, mc._edge_perm(len(col), perm) if aggr == "add" else None)
        dp = _depth_perm(h.shape[1], perm)
        w_l, w_r = g("convs.%d.lin_l.weight" % i), g("convs.%d.lin_r.weight" % i)
        if dp is None:
            h = agg @ w_l.t() + g("convs.%d.lin_l.bias" % i) + h @ w_r.t()
        else:
            h = agg[:, dp] @ w_l[:, dp].t() + g("convs.%d.lin_l.bias" % i) + h[:, dp] @ w_r[:, dp].t()
        if i < hops - 1:
            h = ((h - g("bns.%d.running_mean" % i)) / torch.sqrt(g("bns.%d.running_var" % i) + mc.EPS) * g("bns.%d.weight" % i)
                 + g("bns.%d.bias" % i)).relu()
    return h


def eval_yardstick(state: dict, hops: int, aggr: str):
    ref = run_eval(state, hops, torch.float64, aggr)
    return ref, FACTOR * max(max(err(run_eval(state, hops, torch.float32, aggr, perm), ref) for perm in range(PERMS)), FLOOR)
