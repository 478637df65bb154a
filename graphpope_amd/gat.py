"""Full-batch GAT on the HIP kernels of csrc/gat.h: the attention layer over the ``features (+) POPE`` tensor.

``GATConv`` follows PyG 1.7.0's ``GATConv(in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
add_self_loops=True, bias=True)`` on a single ``x`` [3p: PyG is not installed here, parity unpinned]: ``h = lin_l(x)`` viewed
``[N, H, C]`` (``lin_r`` is the same module), per-edge scores ``leaky_relu(<h_j, att_l> + <h_i, att_r>)``, a softmax over every
destination's in-edges, and the weighted sum.  Parameters are ``lin_l.weight [H * C, in_channels]``, ``att_l`` and ``att_r``
``[1, H, C]`` and ``bias``.  The projection, the scores, the edge softmax, the propagate and every gradient run in libgraphpope_hip.so
(pope_gat_*; include/graphpope_hip.h states the summation order); there is no CPU path.  Attention dropout is not implemented:
``dropout > 0`` in training mode raises ``NotImplementedError``.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._lib import check, on_device, ptr
from .gcn import GraphAdj, _bytes
from .sage import _stream

__all__ = ["GATConv", "GAT", "GraphAdj"]


def _glorot(t):
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    nn.init.uniform_(t, -a, a)


class _GatConvFn(torch.autograd.Function):
    """One autograd node around pope_gat_conv_forward / pope_gat_conv_backward.  What the backward pass needs (h, a_src, a_dst, alpha,
    alpha_self) is written by the forward call into tensors of this node and saved; nothing hangs on the tensors themselves."""

    @staticmethod
    def forward(ctx, x, weight, att_l, att_r, bias, adj, heads, concat, negative_slope, add_self_loops):
        if not (x.is_cuda and weight.is_cuda):
            raise RuntimeError("GATConv runs on the GPU only (no CPU fallback)")
        lib = _lib.load()
        x, w = x.contiguous().float(), weight.contiguous()
        al, ar = att_l.contiguous(), att_r.contiguous()
        b = None if bias is None else bias.contiguous()
        n, c_in, H = adj.num_nodes, w.shape[1], int(heads)
        C = w.shape[0] // H
        if x.shape != (n, c_in):
            raise ValueError(f"GATConv: x is {tuple(x.shape)}, the graph has {n} nodes and the layer {c_in} input channels")
        dev = x.device
        with on_device(dev):
            h = torch.empty((n, H * C), dtype=torch.float32, device=dev)
            a_src, a_dst, alpha_self = (torch.empty((n, H), dtype=torch.float32, device=dev) for _ in range(3))
            alpha = torch.empty((adj.nnz, H), dtype=torch.float32, device=dev)
            out = torch.empty((n, H * C if concat else C), dtype=torch.float32, device=dev)
            scratch = _bytes(lib.pope_gat_conv_forward_scratch_size(n, adj.nnz, c_in, H, C, int(concat)), dev)
            check(lib.pope_gat_conv_forward(ptr(adj.rowptr), ptr(adj.col), n, adj.nnz, ptr(x), c_in, ptr(w), ptr(al), ptr(ar), ptr(b), H, C,
                                            int(concat), negative_slope, int(add_self_loops), ptr(h), ptr(a_src), ptr(a_dst),
                                            ptr(alpha) if adj.nnz else None, ptr(alpha_self), ptr(out), ptr(scratch), scratch.numel(), _stream()))
        ctx.save_for_backward(x, w, al, ar, h, a_src, a_dst, alpha, alpha_self)
        ctx.adj, ctx.conf, ctx.has_bias = adj, (H, C, bool(concat), float(negative_slope), bool(add_self_loops)), b is not None
        ctx.mark_non_differentiable(alpha, alpha_self)
        return out, alpha, alpha_self

    @staticmethod
    def backward(ctx, grad_out, _grad_alpha, _grad_alpha_self):
        lib, adj = _lib.load(), ctx.adj
        x, w, al, ar, h, a_src, a_dst, alpha, alpha_self = ctx.saved_tensors
        H, C, concat, slope, self_loops = ctx.conf
        g = grad_out.contiguous().float()
        n, c_in, dev = adj.num_nodes, w.shape[1], x.device
        with on_device(dev):
            slot_map = adj.slot_map
            grad_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            grad_w, grad_al, grad_ar = torch.empty_like(w), torch.empty_like(al), torch.empty_like(ar)
            grad_b = torch.empty(H * C if concat else C, dtype=torch.float32, device=dev) if ctx.has_bias else None
            scratch = _bytes(lib.pope_gat_conv_backward_scratch_size(n, adj.nnz, c_in, H, C, int(concat)), dev)
            nz = adj.nnz > 0
            check(lib.pope_gat_conv_backward(ptr(adj.rowptr), ptr(adj.col), ptr(adj.rowptr_t), ptr(adj.col_t), ptr(slot_map), n, adj.nnz, ptr(x),
                                             c_in, ptr(w), ptr(al), ptr(ar), H, C, int(concat), slope, int(self_loops), ptr(h), ptr(a_src),
                                             ptr(a_dst), ptr(alpha) if nz else None, ptr(alpha_self), ptr(g), ptr(grad_x), ptr(grad_w),
                                             ptr(grad_al), ptr(grad_ar), ptr(grad_b), ptr(scratch), scratch.numel(), _stream()))
        return grad_x, grad_w, grad_al, grad_ar, grad_b, None, None, None, None, None


class GATConv(nn.Module):
    """``conv(x, adj)`` over the whole graph, ``adj`` a :class:`GraphAdj`: PyG 1.7.0's ``GATConv`` on a single ``x`` [3p, parity
    unpinned].

    With ``add_self_loops`` the self-loop slots of the graph are skipped and every node attends to itself once (the diagonal is replaced,
    as in ``GCNConv``); without, self-loop slots are ordinary edges and a node without in-edges gets ``bias`` alone.  Repeated edges are
    separate terms of the softmax.  ``concat=True`` gives ``[N, heads * out_channels]``, ``concat=False`` the mean over the heads.
    ``forward(..., return_attention_weights=True)`` also returns ``(alpha [nnz, heads], alpha_self [N, heads])``: the attention of every
    slot of ``adj.col`` (0 for a skipped slot) and of the self term (0 without self loops)."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True, negative_slope: float = 0.2,
                 dropout: float = 0.0, add_self_loops: bool = True, bias: bool = True):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = int(in_channels), int(out_channels), int(heads)
        if self.in_channels < 1 or self.out_channels < 1 or self.heads < 1:
            raise ValueError("GATConv: in_channels, out_channels and heads must be positive")
        self.concat, self.negative_slope, self.dropout = bool(concat), float(negative_slope), float(dropout)
        if not (0.0 <= self.negative_slope <= 1.0):
            raise ValueError(f"GATConv: negative_slope {negative_slope} is not in [0, 1]")
        self.add_self_loops = bool(add_self_loops)
        self.lin_l = nn.Linear(self.in_channels, self.heads * self.out_channels, bias=False)
        self.att_l = nn.Parameter(torch.empty(1, self.heads, self.out_channels))
        self.att_r = nn.Parameter(torch.empty(1, self.heads, self.out_channels))
        self.bias = nn.Parameter(torch.empty(self.heads * self.out_channels if self.concat else self.out_channels)) if bias else None
        self.reset_parameters()

    @property
    def lin_r(self):
        """PyG 1.7.0 on a single ``x``: the same module as ``lin_l`` (not registered twice: the state dict holds ``lin_l.weight`` alone)."""
        return self.lin_l

    def reset_parameters(self):
        _glorot(self.lin_l.weight)
        _glorot(self.att_l)
        _glorot(self.att_r)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x: torch.Tensor, adj: GraphAdj, return_attention_weights: bool = False):
        if self.dropout > 0.0 and self.training:
            raise NotImplementedError(f"GATConv: dropout={self.dropout} in training mode (attention dropout) is not implemented")
        if not x.is_cuda:
            raise RuntimeError("GATConv runs on the GPU only (no CPU fallback)")
        out, alpha, alpha_self = _GatConvFn.apply(x, self.lin_l.weight, self.att_l, self.att_r, self.bias, adj, self.heads, self.concat,
                                                  self.negative_slope, self.add_self_loops)
        return (out, (alpha, alpha_self)) if return_attention_weights else out

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, heads={self.heads}"


class GAT(nn.Module):
    """``num_layers`` GATConv layers over the whole graph: ``dropout -> conv -> elu`` per layer on the features.  The hidden convs are
    ``GATConv(., hidden_channels // heads, heads)`` (concatenated: ``hidden_channels`` wide), the last conv has one head and no ELU.
    Dropout and ELU are torch's own ops; the convs' attention dropout is 0.  (``gatv2.GATv2`` is this stack over ``GATv2Conv``.)"""

    conv_class = GATConv

    def __init__(self, in_channels: int, hidden_channels: int, out_channels: int, num_layers: int = 2, heads: int = 8, dropout: float = 0.5,
                 **conv_kwargs):
        super().__init__()
        name = type(self).__name__
        if num_layers < 1:
            raise ValueError(f"{name}: num_layers must be at least 1")
        if heads < 1 or hidden_channels % heads:
            raise ValueError(f"{name}: hidden_channels {hidden_channels} is not a multiple of heads {heads}")
        convs, width = [], in_channels
        for _ in range(num_layers - 1):
            convs.append(self.conv_class(width, hidden_channels // heads, heads, **conv_kwargs))
            width = hidden_channels
        convs.append(self.conv_class(width, out_channels, 1, **conv_kwargs))
        self.convs = nn.ModuleList(convs)
        self.dropout = float(dropout)

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def forward(self, x: torch.Tensor, adj: GraphAdj) -> torch.Tensor:
        for i, conv in enumerate(self.convs):
            x = F.dropout(x, p=self.dropout, training=self.training)
            x = conv(x, adj)
            if i < len(self.convs) - 1:
                x = F.elu(x)
        return x
