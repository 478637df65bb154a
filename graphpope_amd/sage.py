"""GraphSAGE on the HIP SAGEConv kernels: the consumer of the ``features (+) POPE`` tensor.

Mirrors /root/reference/main.py:182-211 (class SAGE: ModuleList of SAGEConv + BatchNorm1d, forward
over the sampled ``adjs``) with the PyG ``SAGEConv`` replaced by :class:`SAGEConv` below, whose
neighbour gather + mean and both projections run in libgraphpope_hip.so (fp32, exact-f32 MFMA).
Parameter names follow PyG 1.7.0 (``lin_l.weight``, ``lin_l.bias``, ``lin_r.weight``) so the
reference's Lightning checkpoints stay loadable.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._lib import AGGR, check, on_device, ptr


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def set_deterministic(on: bool) -> bool:
    """Deterministic mode of the library (sage_set_deterministic): returns the previous value.

    Off (the default): the input gradient of a hidden SAGEConv is scattered with float atomics, so two runs of a training step on the
    same inputs may differ in their last bits.  On: that gradient is summed per source row in a fixed order and ``EvalMetrics.update``
    adds once per launch; training and evaluation steps are then pure functions of their inputs (weights, batch, seeds).  Process-wide,
    needs no device.  The setting is read when a layer's backward pass is enqueued: a captured HIP graph keeps the mode it was
    captured under (:class:`graphpope_amd.train.SageTrainStep`)."""
    return bool(_lib.load().sage_set_deterministic(1 if on else 0))


def is_deterministic() -> bool:
    return bool(_lib.load().sage_get_deterministic())


class deterministic:
    """``with sage.deterministic():`` -- :func:`set_deterministic` for the length of the block; the previous value comes back."""

    def __init__(self, on: bool = True):
        self.on = bool(on)

    def __enter__(self):
        self.was = set_deterministic(self.on)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.was)
        return False


class SampledAdj:
    """One bipartite block of a sampled mini-batch: CSR by destination, destinations = first n_dst sources.

    Stands in for the ``torch_sparse.SparseTensor`` ``adj_t`` PyG's NeighborSampler yields
    (main.py:59-63, 118-123): ``size(0)`` = n_dst, ``size(1)`` = n_src, values dropped.

    ``dims`` (device int32 [4] = {n_dst, n_src, nnz, 0}, written by the device-extent sampler) makes the block one of
    DEVICE extents: ``n_dst`` / ``n_src`` / the lengths of ``rowptr`` and ``col`` are then capacities, the kernels read the
    true sizes from ``dims`` and nothing is ever read back to the host (include/graphpope_hip.h, "Device extents").
    """

    def __init__(self, rowptr: torch.Tensor, col: torch.Tensor, n_src: int, dims: torch.Tensor | None = None):
        self.rowptr = rowptr.to(torch.int32).contiguous()
        self.col = col.to(torch.int32).contiguous()
        self.n_dst = int(rowptr.numel() - 1)
        self.n_src = int(n_src)
        if dims is not None:
            assert dims.is_cuda and dims.dtype == torch.int32 and dims.numel() >= 3 and dims.is_contiguous()
        self.dims = dims

    def size(self, dim: int) -> int:
        return (self.n_dst, self.n_src)[dim]

    def to(self, device):
        return SampledAdj(self.rowptr.to(device), self.col.to(device), self.n_src, None if self.dims is None else self.dims.to(device))

    def device_extents(self) -> "SampledAdj":
        """The same block with its sizes in a device word triple (for blocks sampled on the host: pools of pre-sampled
        batches that feed a replayed step)."""
        if self.dims is not None:
            return self
        dims = torch.tensor([self.n_dst, self.n_src, int(self.col.numel()), 0], dtype=torch.int32, device=self.rowptr.device)
        return SampledAdj(self.rowptr, self.col, self.n_src, dims)


def _forward_scratch(lib, n_dst, c_in, c_out, dev):
    """Partial-tile slabs of the stream-K forward projection (None, 0 for layers too small to use it).  Taken from
    torch's caching allocator per call: stream-ordered like every other buffer of the step."""
    nbytes = lib.sage_conv_forward_scratch_bytes(n_dst, c_in, c_out)
    if nbytes == 0:
        return None, 0
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _stats_buffers(n_dst, c_out, dev):
    """Room for the per-row-tile column sums the projection's epilogue leaves for BatchNorm (sage_conv_forward_stats): float64
    [2, ceil(n_dst / 16), c_out] on the device and the two host ints the call reports (tiles written, rows per tile)."""
    return torch.empty((2, (n_dst + 15) // 16, c_out), dtype=torch.float64, device=dev), (ctypes.c_int32 * 2)(0, 0)


L2_EPS = 1e-12          # torch.nn.functional.normalize's default, the one PyG's SAGEConv.forward normalises with


def _l2_normalize_(lib, out, rows_dev):
    """F.normalize(out, p=2., dim=-1) of the contiguous `out` IN PLACE (csrc/l2norm.hip): the reciprocal norms, float32 [M], that the
    backward pass reads beside the normalised rows.  `rows_dev`: the block's device extents (their first word is the row count) or None."""
    inv_norm = torch.empty(out.shape[0], dtype=torch.float32, device=out.device)
    check(lib.sage_l2_normalize_forward(ptr(out), out.shape[0], out.shape[1], L2_EPS, ptr(out), ptr(inv_norm), ptr(rows_dev), _stream()))
    return inv_norm


def _l2_normalize_backward(lib, y, inv_norm, grad_y, rows_dev, in_place):
    """The gradient in front of :func:`_l2_normalize_` for the contiguous `grad_y`.  `in_place`: written over `grad_y` -- only for a
    tensor the caller made itself; a gradient autograd handed in may be shared with other nodes."""
    grad_x = grad_y if in_place else torch.empty_like(grad_y)
    check(lib.sage_l2_normalize_backward(ptr(y), ptr(inv_norm), ptr(grad_y), y.shape[0], y.shape[1], L2_EPS, ptr(grad_x), ptr(rows_dev), _stream()))
    return grad_x


class IndexedFeatures:
    """``Batch.x = data.x[n_id]`` (main.py:118-123) WITHOUT the copy: the resident feature matrix plus the batch's node
    ids.  Passed to :class:`SAGE` / :class:`SAGEConv` in place of the gathered ``x``, the first layer reads its
    neighbours' rows straight from ``feats`` (sage_conv_forward_indexed); only the destination rows are materialised."""

    def __init__(self, feats: torch.Tensor, n_id: torch.Tensor):
        assert feats.dim() == 2 and feats.dtype == torch.float32 and feats.is_contiguous() and not feats.requires_grad
        assert n_id.dtype == torch.int64 and n_id.dim() == 1 and n_id.device == feats.device
        self.feats, self.n_id = feats, n_id.contiguous()

    def materialize(self) -> torch.Tensor:
        return self.feats.index_select(0, self.n_id)


def _check_aggr(aggr):
    if aggr not in AGGR:
        raise ValueError(f"aggr={aggr!r}: expected 'mean', 'add' or 'max'")
    return aggr


def _conv_forward(lib, x, w_l, b_l, w_r, adj, want_stats, normalize=False, aggr='mean', want_arg=False):
    """The layer's forward launches for `x` = the source rows [n_src, c_in] or an :class:`IndexedFeatures`.  Returns the output
    [n_dst, c_out], the four tensors the backward pass reads (rows, agg, w_l, w_r) and, if `want_stats` and the kernels of this shape
    produce them, the first stage of the output's BatchNorm statistics as (partials, tiles, rows per tile), else None.

    `normalize`: the output's rows are L2-normalised where they lie (one more launch; the un-normalised output is not kept) and a fifth
    tensor is kept, the reciprocal norms.  The projection's statistics describe the un-normalised matrix, so none are produced.

    `aggr`: 'mean' runs the entry points it always ran; 'add' / 'max' run sage_conv_forward(_indexed)_aggr (csrc/aggregate.hip in the
    gather's place, the same projections and statistics).  `want_arg` ('max' only; never behind an :class:`IndexedFeatures`, whose matrix
    takes no gradient): the winning sources, int32 [n_dst, c_in], are recorded and kept behind w_r for the backward pass."""
    want_stats = want_stats and not normalize
    indexed = isinstance(x, IndexedFeatures)
    feats = x.feats if indexed else x
    if not feats.is_cuda:
        raise RuntimeError("SAGEConv runs on the GPU only (no CPU fallback)")
    if not (feats.is_contiguous() and w_l.is_contiguous() and w_r.is_contiguous()):
        feats, w_l, w_r = feats.contiguous(), w_l.contiguous(), w_r.contiguous()
    rowptr, col, n_dst, dev = adj.rowptr, adj.col, adj.size(0), feats.device
    c_in, c_out = feats.shape[1], w_l.shape[0]
    agg = torch.empty((n_dst, c_in), dtype=torch.float32, device=dev)
    x_dst = torch.empty((n_dst, c_in), dtype=torch.float32, device=dev) if indexed else None
    out = torch.empty((n_dst, c_out), dtype=torch.float32, device=dev)
    with on_device(dev):
        scratch, nbytes = _forward_scratch(lib, n_dst, c_in, c_out, dev)
        if indexed:                                   # neighbours read through n_id, the destination rows written out as x_dst
            plain, with_stats = lib.sage_conv_forward_indexed, lib.sage_conv_forward_indexed_stats
            args = (ptr(rowptr), ptr(col), ptr(x.n_id), x.n_id.numel(), n_dst, col.numel(), ptr(feats), feats.shape[0], c_in, ptr(w_l),
                    ptr(b_l), ptr(w_r), c_out, ptr(agg), ptr(x_dst), ptr(out), ptr(scratch), nbytes, ptr(adj.dims))
        else:
            plain, with_stats = lib.sage_conv_forward, lib.sage_conv_forward_stats
            args = (ptr(rowptr), ptr(col), feats.shape[0], n_dst, col.numel(), ptr(feats), c_in, ptr(w_l), ptr(b_l), ptr(w_r), c_out,
                    ptr(agg), ptr(out), ptr(scratch), nbytes, ptr(adj.dims))
        stats, arg = None, ()
        if aggr != 'mean':                            # one entry point with or without the statistics, then the aggregator and its arg
            with_aggr = lib.sage_conv_forward_indexed_aggr if indexed else lib.sage_conv_forward_aggr
            if aggr == 'max' and want_arg and not indexed:
                arg = (torch.empty((n_dst, c_in), dtype=torch.int32, device=dev),)
            plain = lambda *a: with_aggr(*a[:-1], None, None, 0, None, AGGR[aggr], ptr(arg[0] if arg else None), a[-1])
            with_stats = lambda *a: with_aggr(*a[:-1], AGGR[aggr], ptr(arg[0] if arg else None), a[-1])
        if want_stats:                                # the projection's epilogue leaves the first stage of the BatchNorm statistics of `out`
            partials, info = _stats_buffers(n_dst, c_out, dev)
            check(with_stats(*args, ptr(partials[0]), ptr(partials[1]), partials.shape[1], info, _stream()))
            if info[0] > 0:
                stats = (partials, int(info[0]), int(info[1]))
        else:
            check(plain(*args, _stream()))
        inv_norm = (_l2_normalize_(lib, out, adj.dims),) if normalize else ()
    # x_dst is kept as a matrix for the backward pass: reading the destination rows through n_id in the weight-gradient kernel
    # (sage_conv_backward_indexed) was measured 29 us slower per step than the 60 MB this copy costs
    return out, (x_dst if indexed else feats, agg, w_l, w_r, *arg, *inv_norm), stats


def _conv_backward(lib, rows, agg, w_l, w_r, adj, grad_out, need_x, need_b, aggr='mean', arg=None):
    """sage_conv_backward over what :func:`_conv_forward` kept: (grad_x, grad_w_l, grad_b_l, grad_w_r), with grad_x / grad_b_l None
    unless asked for.  `rows` = the source rows, or the destination rows alone behind an :class:`IndexedFeatures` (the call then runs
    with n_src = n_dst, and `need_x` is False: the feature matrix takes no gradient).  `grad_out`: the gradient of the projection's
    output -- behind a normalising conv, what :func:`_l2_normalize_backward` returned.  `aggr` 'add' / 'max': sage_conv_backward_aggr, whose
    input gradient is an ordered sum in either mode of the library; `arg`: what a 'max' forward pass recorded (None without `need_x`)."""
    (n_src, c_in), n_dst, c_out, dev = rows.shape, agg.shape[0], w_l.shape[0], rows.device
    rowptr, col = adj.rowptr, adj.col
    grad_out = grad_out.contiguous()
    grad_x = torch.empty_like(rows) if need_x else None
    grad_w_l, grad_w_r = torch.empty_like(w_l), torch.empty_like(w_r)
    grad_b = torch.empty(c_out, dtype=torch.float32, device=dev) if need_b else None
    with on_device(dev):
        size_of = lib.sage_conv_scratch_bytes if aggr == 'mean' else lib.sage_conv_backward_aggr_scratch_size
        scratch = torch.empty(max(size_of(n_src, n_dst, col.numel(), c_in, c_out), 16), dtype=torch.uint8, device=dev)
        args = (ptr(rowptr), ptr(col), n_src, n_dst, col.numel(), ptr(rows), ptr(agg), c_in, ptr(w_l), ptr(w_r), c_out, ptr(grad_out), ptr(grad_x),
                ptr(grad_w_l), ptr(grad_b), ptr(grad_w_r), ptr(scratch), scratch.numel(), ptr(adj.dims))
        if aggr == 'mean':
            check(lib.sage_conv_backward(*args, _stream()))
        else:
            check(lib.sage_conv_backward_aggr(*args, AGGR[aggr], ptr(arg), _stream()))
    return grad_x, grad_w_l, grad_b, grad_w_r


class _Tail(NamedTuple):
    """What one BatchNorm1d -> ReLU -> dropout call needs beside x, gamma and beta (:func:`_tail_of`)."""
    running_mean: torch.Tensor | None
    running_var: torch.Tensor | None
    num_batches_tracked: torch.Tensor | None      # counted up inside the statistics kernel; None: not counted there
    momentum: float
    eps: float
    batch_stats: bool                             # normalise with the batch's statistics (training, or no running ones)
    p: float
    seed: int
    rows: torch.Tensor | None
    seed_dev: torch.Tensor | None


def _bn_forward(lib, x, gamma, beta, t: _Tail, stats=None):
    """BatchNorm1d -> ReLU -> dropout of the contiguous `x` (csrc/epilogue.hip): (y, mean, rstd).  `stats`: the first stage of the batch
    statistics as :func:`_conv_forward` returns it -- the pass over `x` that computes it is then not launched."""
    if not x.is_cuda:
        raise RuntimeError("the fused BatchNorm/ReLU/dropout epilogue runs on the GPU only (no CPU fallback)")
    (m, c), dev = x.shape, x.device
    y = torch.empty_like(x)
    mean = torch.empty(c, dtype=torch.float32, device=dev)
    rstd = torch.empty(c, dtype=torch.float32, device=dev)
    with on_device(dev):
        scratch = torch.empty(lib.sage_bn_scratch_bytes(c), dtype=torch.uint8, device=dev)
        args = (ptr(x), m, c, ptr(gamma), ptr(beta), ptr(t.running_mean), ptr(t.running_var), ptr(t.num_batches_tracked), t.momentum, t.eps,
                int(t.batch_stats), t.p, t.seed, ptr(y), ptr(mean), ptr(rstd), ptr(scratch), scratch.numel(), ptr(t.rows), ptr(t.seed_dev))
        if stats is None:
            check(lib.sage_bn_relu_dropout_forward(*args, _stream()))
        else:
            partials, tiles, rows_per_tile = stats
            check(lib.sage_bn_relu_dropout_forward_stats(*args, ptr(partials[0]), ptr(partials[1]), tiles, rows_per_tile, _stream()))
    return y, mean, rstd


def _bn_backward(lib, x, gamma, beta, mean, rstd, t: _Tail, grad_y, sum_columns):
    """(grad_x, grad_gamma, grad_beta, colsum) of :func:`_bn_forward`.  `sum_columns`: also the column sums of grad_x (float32 [C]) out
    of the statistics pass's float64 sums -- the bias gradient of the layer that produced `x`, which would otherwise take that layer
    a launch that reads grad_x back; else colsum is None."""
    (m, c), dev = x.shape, x.device
    grad_y = grad_y.contiguous()
    grad_x = torch.empty_like(x)
    grad_gamma = torch.empty_like(gamma)
    grad_beta = torch.empty_like(beta)
    with on_device(dev):
        scratch = torch.empty(lib.sage_bn_scratch_bytes(c), dtype=torch.uint8, device=dev)
        args = (ptr(x), ptr(grad_y), m, c, ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), int(t.batch_stats), t.p, t.seed, ptr(grad_x),
                ptr(grad_gamma), ptr(grad_beta), ptr(scratch), scratch.numel(), ptr(t.rows), ptr(t.seed_dev))
        colsum = None
        if sum_columns:
            colsum = torch.empty(c, dtype=torch.float32, device=dev)
            check(lib.sage_bn_relu_dropout_backward_bias(*args, ptr(colsum), _stream()))
        else:
            check(lib.sage_bn_relu_dropout_backward(*args, _stream()))
    return grad_x, grad_gamma, grad_beta, colsum


class _SageConvFn(torch.autograd.Function):
    """SAGEConv on its own: the last layer, or a conv whose output the caller wants to see."""

    @staticmethod
    def forward(ctx, x, w_l, b_l, w_r, adj, normalize=False, aggr='mean'):
        out, kept, _ = _conv_forward(_lib.load(), x, w_l, b_l, w_r, adj, False, normalize, aggr, ctx.needs_input_grad[0])
        ctx.save_for_backward(*kept, *((out,) if normalize else ()))
        ctx.adj, ctx.has_bias, ctx.normalize, ctx.aggr = adj, b_l is not None, bool(normalize), aggr
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib, kept = _lib.load(), ctx.saved_tensors
        if ctx.normalize:                    # through the normalisation first: kept = (rows, agg, w_l, w_r, [arg,] inv_norm, y)
            *kept, inv_norm, y = kept
            with on_device(y.device):
                grad_out = _l2_normalize_backward(lib, y, inv_norm, grad_out.contiguous(), ctx.adj.dims, in_place=False)
        grad_x, grad_w_l, grad_b, grad_w_r = _conv_backward(lib, *kept[:4], ctx.adj, grad_out, ctx.needs_input_grad[0], ctx.has_bias, ctx.aggr,
                                                            *kept[4:])
        return grad_x, grad_w_l, grad_b, grad_w_r, None, None, None


class _Linear(nn.Module):
    """Weight (+ bias) holder named like torch.nn.Linear so state dicts line up with PyG's lin_l / lin_r."""

    def __init__(self, c_in, c_out, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(c_out, c_in))
        self.bias = nn.Parameter(torch.empty(c_out)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))       # torch.nn.Linear's default
        if self.bias is not None:
            bound = 1 / math.sqrt(self.weight.shape[1])
            nn.init.uniform_(self.bias, -bound, bound)


class SAGEConv(nn.Module):
    """``conv((x_src, x_dst), adj_t)``: PyG 1.7.0's ``SAGEConv(in_channels, out_channels, normalize=False, root_weight=True, bias=True,
    aggr='mean')`` with its parameter names (there ``aggr`` is a keyword of ``MessagePassing``; here it stands behind the positional order).

    ``aggr``: ``'mean'`` (the default), ``'add'`` or ``'max'`` -- what the neighbours' rows are folded with before ``lin_l``
    (``matmul(adj_t, x, reduce=aggr)``).  Sum and max run csrc/aggregate.hip in the gather's place, forward and backward; an empty row
    aggregates to 0 under all three; a NaN among a row's neighbours makes its max NaN; the gradient of a max goes to the FIRST slot that holds
    it.  Their input gradient is an ordered sum without float atomics, so both are bit-reproducible whatever :func:`set_deterministic` says.
    Anything else is a ``ValueError``.  The state dict does not depend on ``aggr``.

    ``normalize``: the output rows are L2-normalised, ``F.normalize(out, p=2., dim=-1)`` (line 7 of Algorithm 1 of the GraphSAGE paper),
    by one HIP launch behind the projection and one in front of its backward pass (csrc/l2norm.hip).  ``bias=False``: no ``lin_l.bias``,
    in the module and in its state dict.  ``root_weight=False`` is not implemented: every projection kernel is a product of two
    operands."""

    def __init__(self, in_channels: int, out_channels: int, normalize: bool = False, root_weight: bool = True, bias: bool = True,
                 aggr: str = 'mean'):
        super().__init__()
        self.aggr = _check_aggr(aggr)
        if not root_weight:
            raise NotImplementedError("SAGEConv(root_weight=False): the HIP projection kernels always add lin_r(x_dst); a layer without "
                                      "the root term is not implemented (DESIGN.md §8)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.normalize, self.root_weight = bool(normalize), True
        self.lin_l = _Linear(in_channels, out_channels, bias=bool(bias))
        self.lin_r = _Linear(in_channels, out_channels, bias=False)

    def forward(self, x, adj_t: SampledAdj):
        """``x``: the source rows, ``(x_src, x_dst)`` or an :class:`IndexedFeatures`."""
        if self.aggr != 'mean':
            return _SageConvFn.apply(_source_rows(x), self.lin_l.weight, self.lin_l.bias, self.lin_r.weight, adj_t, self.normalize, self.aggr)
        if not self.normalize:
            return _SageConvFn.apply(_source_rows(x), self.lin_l.weight, self.lin_l.bias, self.lin_r.weight, adj_t)
        return _SageConvFn.apply(_source_rows(x), self.lin_l.weight, self.lin_l.bias, self.lin_r.weight, adj_t, True)


def _source_rows(x):
    return x[0] if isinstance(x, (tuple, list)) else x            # x_dst = x_src[:n_dst] by construction (main.py:206)


class _BnReluDropoutFn(torch.autograd.Function):
    """BatchNorm1d -> ReLU -> dropout (csrc/epilogue.hip, main.py:207-209) of `x` -- or, given `adj`, of the SAGEConv of `x` with the
    conv inside the node (main.py:206-209 as ONE node of the autograd graph).  The two halves then hand each other the BatchNorm
    statistics (forward) and the conv's bias gradient (backward) as local variables; the conv output between them is saved for the
    backward pass and never returned, so no other consumer and no in-place edit can come between a hand-off and the values it was
    computed from.

    A normalising conv (`normalize`) sits between the two halves: BatchNorm then sees the normalised rows, so neither hand-off is valid --
    the projection's statistics describe the un-normalised matrix, and the column sums of the BatchNorm's input gradient are not the
    bias gradient once the normalisation's backward pass stands between them.  The statistics pass then runs over the normalised rows
    and the bias gradient comes from the conv's own backward pass."""

    @staticmethod
    def forward(ctx, x, gamma, beta, tail, w_l=None, b_l=None, w_r=None, adj=None, normalize=False, aggr='mean'):
        lib = _lib.load()
        if adj is None:
            h, kept, stats = x.contiguous(), (), None
        else:
            h, kept, stats = _conv_forward(lib, x, w_l, b_l, w_r, adj, tail.batch_stats, normalize, aggr, ctx.needs_input_grad[0])
        y, mean, rstd = _bn_forward(lib, h, gamma, beta, tail, stats)
        ctx.save_for_backward(h, gamma, beta, mean, rstd, *kept)
        ctx.tail, ctx.adj, ctx.has_bias, ctx.normalize, ctx.aggr = tail, adj, b_l is not None, bool(normalize) and adj is not None, aggr
        ctx.bias_from_tail = stats is not None       # the forward pass took the conv's statistics: the backward pass takes the tail's column sums
        return y

    @staticmethod
    def backward(ctx, grad_y):
        lib = _lib.load()
        h, gamma, beta, mean, rstd, *kept = ctx.saved_tensors
        grad_h, grad_gamma, grad_beta, colsum = _bn_backward(lib, h, gamma, beta, mean, rstd, ctx.tail, grad_y, ctx.bias_from_tail)
        if ctx.adj is None:
            return grad_h, grad_gamma, grad_beta, None
        if ctx.normalize:                            # h is the normalised output; grad_h was made here, so it is overwritten
            *kept, inv_norm = kept
            with on_device(h.device):
                grad_h = _l2_normalize_backward(lib, h, inv_norm, grad_h, ctx.adj.dims, in_place=True)
        given_b = colsum if ctx.has_bias else None
        grad_x, grad_w_l, grad_b, grad_w_r = _conv_backward(lib, *kept[:4], ctx.adj, grad_h, ctx.needs_input_grad[0],
                                                            ctx.has_bias and given_b is None, ctx.aggr, *kept[4:])
        return grad_x, grad_gamma, grad_beta, None, grad_w_l, (given_b if given_b is not None else grad_b), grad_w_r, None, None, None


def _tail_of(bn: nn.BatchNorm1d, p: float, training: bool, seed, rows, seed_dev) -> _Tail:
    """The host side of one BatchNorm1d -> ReLU -> dropout call: which statistics normalise, where the step counter goes up, the
    dropout seed."""
    if bn.weight is None or bn.momentum is None:
        raise NotImplementedError("fused epilogue: affine BatchNorm1d with a fixed momentum only (the reference's default)")
    use_batch_stats = training or bn.running_mean is None
    nbt = bn.num_batches_tracked if (training and bn.track_running_stats and bn.num_batches_tracked is not None) else None
    if nbt is not None and not (nbt.is_cuda and nbt.dtype == torch.int64):
        nbt.add_(1)                                       # a counter the kernel cannot reach: torch's own op
        nbt = None
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (training and p > 0 and seed_dev is None) else 0
    rm = bn.running_mean if bn.track_running_stats else None
    rv = bn.running_var if bn.track_running_stats else None
    return _Tail(rm, rv, nbt, float(bn.momentum), float(bn.eps), use_batch_stats, float(p) if training else 0.0, int(seed), rows, seed_dev)


def bn_relu_dropout(x: torch.Tensor, bn: nn.BatchNorm1d, p: float, training: bool, seed: int | None = None,
                    rows: torch.Tensor | None = None, seed_dev: torch.Tensor | None = None) -> torch.Tensor:
    """``F.dropout(bn(x).relu_(), p, training)`` (main.py:207-209) on the fused HIP epilogue.

    `bn` stays an ordinary ``nn.BatchNorm1d`` (same state-dict keys as the reference's checkpoints); its running
    statistics and ``num_batches_tracked`` are updated as torch does.  The dropout mask is a counter hash of
    (seed, element): `seed` defaults to a draw from torch's global generator, so ``torch.manual_seed`` makes runs
    repeatable; the mask itself is not torch's Philox stream.

    ``rows`` (device int32 scalar): the true row count of ``x`` when its first dimension is a capacity (device-extent
    batches).  ``seed_dev`` (device int64 scalar): added to ``seed`` on the device, so that a replayed HIP graph draws a
    new mask every replay; with it ``seed`` defaults to 0 instead of a draw from torch's generator (which is a host read).
    """
    return _BnReluDropoutFn.apply(x, bn.weight, bn.bias, _tail_of(bn, p, training, seed, rows, seed_dev))


def conv_bn_relu_dropout(conv: SAGEConv, bn: nn.BatchNorm1d, x, adj_t: SampledAdj, p: float, training: bool, seed: int | None = None,
                         rows: torch.Tensor | None = None, seed_dev: torch.Tensor | None = None) -> torch.Tensor:
    """``bn_relu_dropout(conv(x, adj_t), bn, p, training, ...)`` (main.py:206-209) as one autograd node, with the same arguments.

    When `bn` normalises with the batch's statistics, the projection's epilogue produces their first stage (one launch less) and the
    BatchNorm backward pass produces the conv's bias gradient (one launch less), at every shape whose kernels can; the results are
    those of the two separate calls up to the order of float64 additions.  The conv output itself is not available: a caller that
    needs it as well makes the two calls.  Behind a conv with ``normalize=True`` neither hand-off exists (:class:`_BnReluDropoutFn`)."""
    if conv.aggr != 'mean':
        return _BnReluDropoutFn.apply(_source_rows(x), bn.weight, bn.bias, _tail_of(bn, p, training, seed, rows, seed_dev),
                                      conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight, adj_t, conv.normalize, conv.aggr)
    return _BnReluDropoutFn.apply(_source_rows(x), bn.weight, bn.bias, _tail_of(bn, p, training, seed, rows, seed_dev),
                                  conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight, adj_t, conv.normalize)


_BAD_LABEL = {}          # per device: int32 [1], set to 1 by the kernel when a label is out of range (never cleared here)


def bad_label_flag(device) -> torch.Tensor:
    """Device int32 [1]: non-zero once :func:`cross_entropy` has met a label outside [0, C) that is not ignore_index
    (such rows are left out of the mean, as ignored ones; torch raises a device-side assert instead)."""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _BAD_LABEL:
        _BAD_LABEL[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return _BAD_LABEL[key]


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, unit_upstream=False, loss_in=None):
        lib = _lib.load()
        if not logits.is_cuda:
            raise RuntimeError("cross_entropy runs on the GPU only (no CPU fallback)")
        logits = logits.contiguous()
        n, c = logits.shape
        dev = logits.device
        out = torch.empty(2, dtype=torch.float32, device=dev)                # [loss, 1 / count]
        grad = torch.empty_like(logits)
        rows = torch.empty(n, dtype=torch.float32, device=dev)
        with on_device(dev):
            check(lib.sage_cross_entropy_forward(ptr(logits), ptr(target), n, c, ignore_index, ptr(out), ptr(grad),
                                                 ctypes.c_void_p(out.data_ptr() + 4), ptr(rows), ptr(bad_label_flag(dev)),
                                                 (2 if loss_in is not None else 1) if unit_upstream else 0, _stream()))
        if unit_upstream and loss_in is not None:
            loss_in.fold_loss(rows, out)              # the optimiser's launch finishes the scalar (sage_adam_step_loss)
        ctx.save_for_backward(grad, out)
        ctx.unit_upstream = bool(unit_upstream)
        return out[0]

    @staticmethod
    def backward(ctx, grad_loss):
        lib = _lib.load()
        grad, out = ctx.saved_tensors
        if ctx.unit_upstream:                 # the forward launch already produced d(mean loss) / d(logits): nothing to launch
            return grad, None, None, None, None
        n, c = grad.shape
        grad_loss = grad_loss.contiguous()
        res = torch.empty_like(grad)
        with on_device(grad.device):
            check(lib.sage_cross_entropy_backward(ptr(grad), n, c, ptr(grad_loss), ctypes.c_void_p(out.data_ptr() + 4), ptr(res),
                                                  _stream()))
        return res, None, None, None, None


def cross_entropy(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -100, unit_upstream: bool = False, loss_in=None) -> torch.Tensor:
    """``F.cross_entropy(logits, target)`` (main.py:216: mean over the rows, integer labels) in two launches forward and
    one backward: the softmax - onehot gradient is produced with the loss and only scaled in the backward pass.

    ``unit_upstream=True`` is a promise that the loss is the root of the backward pass and is seeded with a gradient of 1
    (``loss.backward()``): the whole forward pass is then ONE launch that also scales the gradient by 1 / count, and the
    backward pass launches nothing.  Any other upstream gradient would be ignored -- only a training step that owns its
    ``backward()`` call (graphpope_amd.train.SageTrainStep) sets it.

    ``loss_in`` (a graphpope_amd.optim.Adam, with ``unit_upstream``): the last stage of the forward pass -- the mean of the row
    losses -- becomes one more block of that optimiser's next ``step()`` launch instead of a launch of its own in front of the
    backward pass; the returned scalar is valid once that step has run (round 5: one launch and one kernel boundary less per step)."""
    if (target.dtype != torch.int64 or target.dim() != 1 or logits.dim() != 2 or target.shape[0] != logits.shape[0]
            or logits.dtype != torch.float32):                          # the library reads the raw pointer as float32
        raise ValueError("cross_entropy: logits [N, C] float32 and int64 labels [N] expected")
    if loss_in is not None and not unit_upstream:
        raise ValueError("cross_entropy: loss_in needs unit_upstream=True (a step that owns its backward() and step() calls)")
    return _CrossEntropyFn.apply(logits, target.contiguous(), int(ignore_index), bool(unit_upstream), loss_in)


class EvalMetrics:
    """Loss and accuracy of a pass, accumulated on the device (main.py:216-217, 227-228, 238: ``F.cross_entropy(y_hat, y)`` and
    ``Accuracy()(y_hat.softmax(-1), y)`` of every step, averaged over the pass).  ``update`` is one launch (sage_eval_metrics) that
    adds a batch's loss sum, correct count and row count into three device words; ``read`` is the only read-back, one 24-byte copy.

    ``acc``: the three words, as a device int64 [3] view the caller owns (a replayed step keeps them next to its other state words);
    word 0 holds the bits of the float64 loss sum."""

    def __init__(self, device, acc: torch.Tensor | None = None):
        self.device = torch.device(device)
        if acc is None:
            acc = torch.zeros(3, dtype=torch.int64, device=self.device)
        assert acc.is_cuda and acc.dtype == torch.int64 and acc.numel() == 3 and acc.is_contiguous() and acc.data_ptr() % 8 == 0
        self.acc = acc

    def reset(self) -> None:
        self.acc.zero_()

    def update(self, logits: torch.Tensor, y: torch.Tensor, ignore_index: int = -100) -> None:
        """Add the rows of `logits` (float32 [M, C] on the device) with labels `y` (int64 [M]).  Rows whose label is `ignore_index` or
        outside [0, C) add nothing; the latter set :func:`bad_label_flag`, as in :func:`cross_entropy`."""
        if not logits.is_cuda:
            raise RuntimeError("EvalMetrics runs on the GPU only (no CPU fallback)")
        if logits.dim() != 2 or logits.dtype != torch.float32 or y.dtype != torch.int64 or y.dim() != 1 or y.shape[0] != logits.shape[0]:
            raise ValueError("EvalMetrics.update: logits [M, C] float32 and int64 labels [M] expected")
        logits, y = logits.detach().contiguous(), y.contiguous()
        with on_device(logits.device):
            check(_lib.load().sage_eval_metrics(ptr(logits), ptr(y), logits.shape[0], logits.shape[1], int(ignore_index), ptr(self.acc),
                                                ptr(bad_label_flag(logits.device)), _stream()))

    def read(self):
        """(mean loss, accuracy, rows) of everything added since the last reset; (nan, nan, 0) when no row was counted."""
        words = self.acc.cpu().numpy()
        loss_sum, correct, rows = float(words[:1].view(np.float64)[0]), int(words[1]), int(words[2])
        if rows == 0:
            return float("nan"), float("nan"), 0
        return loss_sum / rows, correct / rows, rows

    def all_reduce(self, group=None) -> None:
        """Data-parallel passes (graphpope_amd.parallel): the three words summed over the ranks of `group`, the loss sum as float64, correct
        and rows as int64 -- the words, never per-rank means, so :meth:`read` gives the mean over all rows of all ranks."""
        import torch.distributed as dist
        dist.all_reduce(self.acc[0:1].view(torch.float64), op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.acc[1:3], op=dist.ReduceOp.SUM, group=group)


class SAGE(nn.Module):
    """main.py:182-211 without the Lightning plumbing.  Keeps the reference's depth quirk: ``forward`` iterates over
    the sampled adjs (two of them, sizes=[25, 10]), so with num_layers=3 the last conv / bn are never executed and
    the logits are hidden_channels wide (SURVEY.md §7 trap 7).

    ``normalize`` and ``aggr`` go to every conv, the last one included, as models written against PyG pass them (the reference leaves
    both at their defaults)."""

    def __init__(self, in_channels: int, out_channels: int, hidden_channels: int, num_layers: int, dropout: float = 0.5,
                 normalize: bool = False, aggr: str = 'mean'):
        super().__init__()
        self.dropout = dropout
        self.aggr = _check_aggr(aggr)
        self.convs = nn.ModuleList()
        self.convs.append(SAGEConv(in_channels, hidden_channels, normalize=normalize, aggr=aggr))
        for _ in range(num_layers - 2):
            self.convs.append(SAGEConv(hidden_channels, hidden_channels, normalize=normalize, aggr=aggr))
        self.convs.append(SAGEConv(hidden_channels, out_channels, normalize=normalize, aggr=aggr))
        self.bns = nn.ModuleList()
        for _ in range(num_layers - 1):
            self.bns.append(nn.BatchNorm1d(hidden_channels))
        self.dropout_seed_dev = None     # device int64 scalar the dropout seeds follow (train.SageTrainStep sets it: graph replay)

    def forward(self, x, adjs):
        for i, adj_t in enumerate(adjs):
            x = x if isinstance(x, IndexedFeatures) else (x, x[:adj_t.size(0)])
            if i == len(adjs) - 1:
                x = self.convs[i](x, adj_t)
                continue
            rows = None if adj_t.dims is None else adj_t.dims[0:1]
            if self.dropout_seed_dev is not None:
                x = conv_bn_relu_dropout(self.convs[i], self.bns[i], x, adj_t, self.dropout, self.training,
                                         seed=0x9E3779B97F4A7C15 * (i + 1) % (1 << 63), rows=rows, seed_dev=self.dropout_seed_dev)
            else:
                x = conv_bn_relu_dropout(self.convs[i], self.bns[i], x, adj_t, self.dropout, self.training, rows=rows)
        return x

    def inference(self, x_all: torch.Tensor, adj_t, hops: int | None = None) -> torch.Tensor:
        """What the model predicts for the graph itself: ``forward`` in eval mode over ALL nodes and ALL their neighbours, no sampling
        (main.py:204-211 with every ``adj_t`` the whole graph).  Returns float32 ``[N, C_last]``.

        ``x_all``: the resident ``[N, F + K]`` float32 matrix.  ``adj_t``: the graph's CSR by destination -- a :class:`SampledAdj` with
        ``n_dst == n_src == N`` or a ``graphpope_amd.engine.Csr`` (``engine.build_csr(edge_index.flip(0), N)``).  ``hops``: how many
        convs run (default: all of them).  Layer ``i < hops - 1`` is conv, BatchNorm on the RUNNING statistics (whatever
        ``self.training`` says) and ReLU; the last is the conv alone -- so ``hops=2`` on a three-layer model gives the hidden-wide
        "logits" the reference trains (the depth quirk of :meth:`forward`).

        Each layer is one sage_full_layer_forward call (project, then gather the projected rows; a pure function of its inputs, bit
        for bit).  A conv with ``normalize=True`` runs that call without its BatchNorm epilogue, then the normalise launch over the result,
        then the evaluation-mode BatchNorm + ReLU by the epilogue entry point :meth:`forward` uses (three more launches per hidden layer).
        A conv with ``aggr`` 'add' or 'max' cannot project first (a max is not linear, and one formulation serves both): each such layer is
        the conv :meth:`forward` runs, over the whole CSR (aggregate, then project), then the same evaluation-mode BatchNorm + ReLU.
        Runs under ``torch.no_grad()``; two ping-pong activation buffers and one scratch allocation per call."""
        lib = _lib.load()
        hops = len(self.convs) if hops is None else int(hops)
        if not 1 <= hops <= len(self.convs):
            raise ValueError(f"SAGE.inference: hops must be in [1, {len(self.convs)}], got {hops}")
        if not x_all.is_cuda:
            raise RuntimeError("SAGE.inference runs on the GPU only (no CPU fallback)")
        if x_all.dim() != 2 or x_all.dtype != torch.float32:
            raise ValueError("SAGE.inference: x_all [N, C] float32 expected")
        n, dev = int(x_all.shape[0]), x_all.device
        rows = adj_t.size(0) if isinstance(adj_t, SampledAdj) else int(adj_t.num_nodes)
        srcs = adj_t.size(1) if isinstance(adj_t, SampledAdj) else rows
        if rows != n or srcs != n or getattr(adj_t, "dims", None) is not None:
            raise ValueError(f"SAGE.inference: adj_t must be the whole graph's CSR over the {n} rows of x_all (host extents)")
        rowptr, col = adj_t.rowptr, adj_t.col
        if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or rowptr.device != dev or col.device != dev:
            raise ValueError("SAGE.inference: int32 rowptr / col on the device of x_all expected")
        nnz = int(col.numel()) if isinstance(adj_t, SampledAdj) else int(adj_t.num_edges)     # (a Csr pads col behind its last edge)
        with torch.no_grad(), on_device(dev):
            x = x_all.contiguous()
            layers = []
            for i in range(hops):
                conv, bn = self.convs[i], (self.bns[i] if i < hops - 1 else None)
                if bn is not None and (bn.running_mean is None or bn.weight is None):
                    raise NotImplementedError("SAGE.inference: affine BatchNorm1d with running statistics only (the reference's default)")
                layers.append((conv, bn, conv.in_channels, conv.out_channels))
            if layers[0][2] != x.shape[1]:
                raise ValueError(f"SAGE.inference: x_all has {x.shape[1]} columns, the first conv takes {layers[0][2]}")
            sizes = [lib.sage_full_layer_scratch_size(n, nnz, c_in, c_out) for _, _, c_in, c_out in layers]
            if any(conv.aggr != 'mean' for conv, _, _, _ in layers):
                if min(sizes) == 0:
                    raise ValueError("SAGE.inference: a shape the library refuses (N and nnz must be below 2**31 - 1)")
                whole = adj_t if isinstance(adj_t, SampledAdj) else SampledAdj(rowptr, col[:nnz], n)
                for conv, bn, _, _ in layers:        # aggregate first: the layer of forward(), every node a destination
                    x = _conv_forward(lib, x, conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight, whole, False, conv.normalize, conv.aggr)[0]
                    if bn is not None:
                        x = _bn_forward(lib, x, bn.weight, bn.bias, _Tail(bn.running_mean, bn.running_var, None, 0.0, float(bn.eps), False,
                                                                         0.0, 0, None, None))[0]
                return x
            if min(sizes) == 0:
                raise ValueError("SAGE.inference: a shape the library refuses (N and nnz must be below 2**31 - 1)")
            scratch = torch.empty(max(sizes), dtype=torch.uint8, device=dev)
            bufs = [torch.empty(n * max([c for j, (_, _, _, c) in enumerate(layers) if j % 2 == k] or [0]), dtype=torch.float32, device=dev)
                    for k in (0, 1)]
            for i, (conv, bn, c_in, c_out) in enumerate(layers):
                out = bufs[i % 2][:n * c_out].view(n, c_out)
                w_l, b_l, w_r = conv.lin_l.weight.contiguous(), conv.lin_l.bias, conv.lin_r.weight.contiguous()
                fused_bn = bn is not None and not conv.normalize          # the normalisation stands between the conv and its BatchNorm
                norm = (bn.weight, bn.bias, bn.running_mean, bn.running_var) if fused_bn else (None,) * 4
                check(lib.sage_full_layer_forward(ptr(rowptr), ptr(col), n, nnz, ptr(x), c_in, ptr(w_l), ptr(b_l), ptr(w_r), c_out,
                                                  *(ptr(t) for t in norm), float(bn.eps) if fused_bn else 0.0, ptr(out), ptr(scratch),
                                                  scratch.numel(), _stream()))
                x = out
                if conv.normalize:               # the layer without its epilogue, the normalise launch, then BatchNorm + ReLU as forward() runs them
                    _l2_normalize_(lib, out, None)
                    if bn is not None:
                        x = _bn_forward(lib, out, bn.weight, bn.bias, _Tail(bn.running_mean, bn.running_var, None, 0.0, float(bn.eps), False,
                                                                           0.0, 0, None, None))[0]
        return x


# ------------------------------------------------------------------------------------------------
# Host-side fan-out sampler for synthetic batches (stands in for PyG NeighborSampler, main.py:100-116).
# Not accelerated; only used to produce Flickr-shaped pre-sampled batches.
# ------------------------------------------------------------------------------------------------
def sample_batch(rowptr: np.ndarray, col: np.ndarray, seeds: np.ndarray, sizes=(25, 10), rng=None):
    """Returns (n_id, adjs) like NeighborSampler: adjs outer -> inner, each a SampledAdj over local ids, and the
    destinations of every block are the first n_dst entries of its sources."""
    rng = rng or np.random.default_rng(0)
    n_id = np.asarray(seeds, dtype=np.int64)
    adjs = []
    for size in sizes:
        local = {int(g): i for i, g in enumerate(n_id)}
        ids = list(n_id)
        rp = [0]
        cols = []
        for g in n_id:
            nbr = col[rowptr[g]:rowptr[g + 1]]
            if nbr.size > size:
                nbr = rng.choice(nbr, size, replace=False)
            for u in nbr:
                u = int(u)
                j = local.get(u)
                if j is None:
                    j = len(ids)
                    local[u] = j
                    ids.append(u)
                cols.append(j)
            rp.append(len(cols))
        adjs.append(SampledAdj(torch.tensor(rp, dtype=torch.int32), torch.tensor(cols, dtype=torch.int32), len(ids)))
        n_id = np.asarray(ids, dtype=np.int64)
    return n_id, adjs[::-1]
