"""Full-batch GATv2 on the HIP kernels of csrc/gatv2.h: the dynamic-attention layer over the ``features (+) POPE`` tensor.

``GATv2Conv`` follows PyG's ``GATv2Conv(in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
add_self_loops=True, bias=True, share_weights=False)`` on a single ``x`` [3p: restated from memory; PyG is not installed here, parity
unpinned]: ``hl = lin_l(x)`` and ``hr = lin_r(x)`` viewed ``[N, H, C]``, per-edge scores ``<att, leaky_relu(hl[j] + hr[i])>``, a softmax
over every destination's in-edges, and the weighted sum of the sources' ``hl`` rows.  Parameters are ``lin_l.weight [H * C,
in_channels]`` and ``lin_l.bias``, the same for ``lin_r`` (with ``share_weights`` ``lin_r`` IS ``lin_l``), ``att [1, H, C]`` and ``bias``
(``bias=False`` drops the linear biases as well, as PyG does).  The projections, the scores, the edge softmax, the propagate and every
gradient run in libgraphpope_hip.so (pope_gatv2_*; include/graphpope_hip.h states the summation order); there is no CPU path.
Attention dropout is not implemented: ``dropout > 0`` in training mode raises ``NotImplementedError``.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._lib import check, on_device, ptr
from .gat import GAT, _glorot
from .gcn import GraphAdj, _bytes
from .sage import _stream

__all__ = ["GATv2Conv", "GATv2", "GraphAdj"]


class _GatV2ConvFn(torch.autograd.Function):
    """One autograd node around pope_gatv2_conv_forward / pope_gatv2_conv_backward.  What the backward pass needs (hl, hr, alpha,
    alpha_self) is written by the forward call into tensors of this node and saved; nothing hangs on the tensors themselves.  With shared
    weights ``weight_r`` / ``bias_r`` are None and hr is hl."""

    @staticmethod
    def forward(ctx, x, weight_l, bias_l, weight_r, bias_r, att, bias, adj, heads, concat, negative_slope, add_self_loops):
        if not (x.is_cuda and weight_l.is_cuda):
            raise RuntimeError("GATv2Conv runs on the GPU only (no CPU fallback)")
        lib = _lib.load()
        cont = lambda t: None if t is None else t.contiguous()                                          # noqa: E731
        x, wl, bl, wr, br, at, b = x.contiguous().float(), cont(weight_l), cont(bias_l), cont(weight_r), cont(bias_r), cont(att), cont(bias)
        share = wr is None
        n, c_in, H = adj.num_nodes, wl.shape[1], int(heads)
        C = wl.shape[0] // H
        if x.shape != (n, c_in):
            raise ValueError(f"GATv2Conv: x is {tuple(x.shape)}, the graph has {n} nodes and the layer {c_in} input channels")
        dev = x.device
        with on_device(dev):
            hl = torch.empty((n, H * C), dtype=torch.float32, device=dev)
            hr = hl if share else torch.empty_like(hl)
            alpha_self = torch.empty((n, H), dtype=torch.float32, device=dev)
            alpha = torch.empty((adj.nnz, H), dtype=torch.float32, device=dev)
            out = torch.empty((n, H * C if concat else C), dtype=torch.float32, device=dev)
            scratch = _bytes(lib.pope_gatv2_conv_forward_scratch_size(n, adj.nnz, c_in, H, C, int(concat)), dev)
            check(lib.pope_gatv2_conv_forward(ptr(adj.rowptr), ptr(adj.col), n, adj.nnz, ptr(x), c_in, ptr(wl), ptr(bl), ptr(wr), ptr(br), ptr(at),
                                              ptr(b), H, C, int(concat), negative_slope, int(add_self_loops), ptr(hl), None if share else ptr(hr),
                                              ptr(alpha) if adj.nnz else None, ptr(alpha_self), ptr(out), ptr(scratch), scratch.numel(), _stream()))
        ctx.save_for_backward(x, wl, wr, at, hl, hr, alpha, alpha_self)
        ctx.adj, ctx.conf = adj, (H, C, bool(concat), float(negative_slope), bool(add_self_loops))
        ctx.has = (bl is not None, br is not None, b is not None)
        ctx.mark_non_differentiable(alpha, alpha_self)
        return out, alpha, alpha_self

    @staticmethod
    def backward(ctx, grad_out, _grad_alpha, _grad_alpha_self):
        lib, adj = _lib.load(), ctx.adj
        x, wl, wr, at, hl, hr, alpha, alpha_self = ctx.saved_tensors
        H, C, concat, slope, self_loops = ctx.conf
        has_bl, has_br, has_b = ctx.has
        share = wr is None
        g = grad_out.contiguous().float()
        n, c_in, dev = adj.num_nodes, wl.shape[1], x.device
        with on_device(dev):
            slot_map = adj.slot_map
            new = lambda like, on=True: torch.empty_like(like) if on else None                          # noqa: E731
            grad_x = new(x, ctx.needs_input_grad[0])
            grad_wl, grad_wr, grad_at = new(wl), new(wl, not share), new(at)
            grad_bl, grad_br = (torch.empty(H * C, dtype=torch.float32, device=dev) if on else None for on in (has_bl, has_br))
            grad_b = torch.empty(H * C if concat else C, dtype=torch.float32, device=dev) if has_b else None
            scratch = _bytes(lib.pope_gatv2_conv_backward_scratch_size(n, adj.nnz, c_in, H, C, int(concat)), dev)
            nz = adj.nnz > 0
            check(lib.pope_gatv2_conv_backward(ptr(adj.rowptr), ptr(adj.col), ptr(adj.rowptr_t), ptr(adj.col_t), ptr(slot_map), n, adj.nnz, ptr(x),
                                               c_in, ptr(wl), ptr(wr), ptr(at), H, C, int(concat), slope, int(self_loops), ptr(hl),
                                               None if share else ptr(hr), ptr(alpha) if nz else None, ptr(alpha_self), ptr(g), ptr(grad_x),
                                               ptr(grad_wl), ptr(grad_bl), ptr(grad_wr), ptr(grad_br), ptr(grad_at), ptr(grad_b), ptr(scratch),
                                               scratch.numel(), _stream()))
        return grad_x, grad_wl, grad_bl, grad_wr, grad_br, grad_at, grad_b, None, None, None, None, None


class GATv2Conv(nn.Module):
    """``conv(x, adj)`` over the whole graph, ``adj`` a :class:`GraphAdj`: PyG's ``GATv2Conv`` on a single ``x`` [3p, restated from
    memory, parity unpinned].

    The terms of a row are ``GATConv``'s: with ``add_self_loops`` the self-loop slots of the graph are skipped and every node attends to
    itself once; without, self-loop slots are ordinary edges and a node without in-edges gets ``bias`` alone.  Repeated edges are separate
    terms of the softmax.  ``concat=True`` gives ``[N, heads * out_channels]``, ``concat=False`` the mean over the heads.
    ``forward(..., return_attention_weights=True)`` also returns ``(alpha [nnz, heads], alpha_self [N, heads])`` in the slot order of
    ``adj.col`` (0 for a skipped slot; ``alpha_self`` 0 without self loops)."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True, negative_slope: float = 0.2,
                 dropout: float = 0.0, add_self_loops: bool = True, bias: bool = True, share_weights: bool = False):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = int(in_channels), int(out_channels), int(heads)
        if self.in_channels < 1 or self.out_channels < 1 or self.heads < 1:
            raise ValueError("GATv2Conv: in_channels, out_channels and heads must be positive")
        self.concat, self.negative_slope, self.dropout = bool(concat), float(negative_slope), float(dropout)
        if not (0.0 <= self.negative_slope <= 1.0):
            raise ValueError(f"GATv2Conv: negative_slope {negative_slope} is not in [0, 1]")
        self.add_self_loops, self.share_weights = bool(add_self_loops), bool(share_weights)
        self.lin_l = nn.Linear(self.in_channels, self.heads * self.out_channels, bias=bool(bias))
        if not self.share_weights:
            self.lin_r = nn.Linear(self.in_channels, self.heads * self.out_channels, bias=bool(bias))
        self.att = nn.Parameter(torch.empty(1, self.heads, self.out_channels))
        self.bias = nn.Parameter(torch.empty(self.heads * self.out_channels if self.concat else self.out_channels)) if bias else None
        self.reset_parameters()

    def __getattr__(self, name):
        # share_weights: lin_r is the same module as lin_l, not registered twice (the state dict holds lin_l.* alone)
        if name == "lin_r" and self.__dict__.get("share_weights"):
            return self.lin_l
        return super().__getattr__(name)

    def reset_parameters(self):
        for lin in (self.lin_l,) if self.share_weights else (self.lin_l, self.lin_r):
            _glorot(lin.weight)
            if lin.bias is not None:
                nn.init.zeros_(lin.bias)
        _glorot(self.att)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x: torch.Tensor, adj: GraphAdj, return_attention_weights: bool = False):
        if self.dropout > 0.0 and self.training:
            raise NotImplementedError(f"GATv2Conv: dropout={self.dropout} in training mode (attention dropout) is not implemented")
        if not x.is_cuda:
            raise RuntimeError("GATv2Conv runs on the GPU only (no CPU fallback)")
        wr, br = (None, None) if self.share_weights else (self.lin_r.weight, self.lin_r.bias)
        out, alpha, alpha_self = _GatV2ConvFn.apply(x, self.lin_l.weight, self.lin_l.bias, wr, br, self.att, self.bias, adj, self.heads,
                                                    self.concat, self.negative_slope, self.add_self_loops)
        return (out, (alpha, alpha_self)) if return_attention_weights else out

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, heads={self.heads}" + (", share_weights=True" if self.share_weights else "")


class GATv2(GAT):
    """``num_layers`` GATv2Conv layers over the whole graph: ``gat.GAT``'s stack (``dropout -> conv -> elu`` per layer) over ``GATv2Conv``.
    The hidden convs are ``GATv2Conv(., hidden_channels // heads, heads)`` (concatenated: ``hidden_channels`` wide), the last conv has one
    head and no ELU.  Dropout and ELU are torch's own ops; the convs' attention dropout is 0."""

    conv_class = GATv2Conv
