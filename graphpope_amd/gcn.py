"""Full-batch GCN on the HIP kernels of csrc/gcn.h: the second consumer of the ``features (+) POPE`` tensor.

``GCNConv`` follows PyG 1.7.0's ``GCNConv(in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True,
bias=True)`` on its ``adj_t`` path [3p: PyG is not installed here, parity unpinned]: ``out = A^ (x W) + b`` with
``A^ = D^-1/2 (A + f I) D^-1/2``, always project first.  Parameters are ``weight [in_channels, out_channels]`` and ``bias
[out_channels]`` (PyG 1.7.0's names; ``lin.*`` is PyG 2.x).  The projection, the propagate and every gradient run in
libgraphpope_hip.so (pope_gcn_*; include/graphpope_hip.h states the summation order); there is no CPU path.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, engine
from ._lib import check, on_device, ptr
from .sage import _stream


def _bytes(n: int, dev) -> torch.Tensor:
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device=dev)


class GraphAdj:
    """The whole graph as the two CSRs a GCN layer needs, built once: by destination (the forward pass: row i lists the sources i sums
    over) and by source (its transpose, the backward pass).  Both come from ``engine.build_csr_canonical``, so every row is ascending
    and the summation order does not depend on the order of ``edge_index``.  ``dinv(improved, add_self_loops)`` is computed on first use
    and kept: ``GCNConv(cached=...)`` has nothing left to cache."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int):
        dev = engine.require_gpu(edge_index.device)
        ei = edge_index.to(dev, torch.int64).contiguous()
        self.num_nodes, self.nnz, self.device = int(num_nodes), int(ei.shape[1]), dev
        if self.num_nodes <= 0:
            raise ValueError("GraphAdj: num_nodes must be positive")
        by_dst = engine.build_csr_canonical(ei.flip(0).contiguous(), self.num_nodes)
        by_src = engine.build_csr_canonical(ei, self.num_nodes)
        self.rowptr, self.col = by_dst.rowptr, by_dst.col
        self.rowptr_t, self.col_t = by_src.rowptr, by_src.col
        self._dinv = {}
        self._slot_map = None

    @property
    def slot_map(self) -> torch.Tensor:
        """int32 [nnz]: for every slot of the CSR by source the slot of the CSR by destination that holds the same edge
        (pope_gat_slot_map; graphpope_amd.gat reads the attention of an edge through it).  Built on first use and kept."""
        if self._slot_map is None:
            out = torch.empty(max(self.nnz, 1), dtype=torch.int32, device=self.device)
            with on_device(self.device):
                check(_lib.load().pope_gat_slot_map(ptr(self.rowptr), ptr(self.col), ptr(self.rowptr_t), ptr(self.col_t), self.num_nodes,
                                                    self.nnz, ptr(out), _stream()))
            self._slot_map = out
        return self._slot_map

    def self_weight(self, improved: bool, add_self_loops: bool) -> float:
        return (2.0 if improved else 1.0) if add_self_loops else 0.0

    def dinv(self, improved: bool = False, add_self_loops: bool = True) -> torch.Tensor:
        """float32 [N]: ``deg^-1/2`` of ``A + f I`` by destination row (pope_gcn_degree_norm), 0 where the degree is 0."""
        key = (bool(improved) and bool(add_self_loops), bool(add_self_loops))
        if key not in self._dinv:
            out = torch.empty(self.num_nodes, dtype=torch.float32, device=self.device)
            with on_device(self.device):
                check(_lib.load().pope_gcn_degree_norm(ptr(self.rowptr), ptr(self.col), self.num_nodes, self.nnz,
                                                       self.self_weight(*key), ptr(out), _stream()))
            self._dinv[key] = out
        return self._dinv[key]


class _GcnConvFn(torch.autograd.Function):
    """One autograd node around pope_gcn_conv_forward / pope_gcn_conv_backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, adj, dinv, self_weight):
        if not (x.is_cuda and weight.is_cuda):
            raise RuntimeError("GCNConv runs on the GPU only (no CPU fallback)")
        lib = _lib.load()
        x, w = x.contiguous().float(), weight.contiguous()
        b = None if bias is None else bias.contiguous()
        n, (c_in, c_out) = adj.num_nodes, w.shape
        if x.shape != (n, c_in):
            raise ValueError(f"GCNConv: x is {tuple(x.shape)}, the graph has {n} nodes and the layer {c_in} input channels")
        with on_device(x.device):
            out = torch.empty((n, c_out), dtype=torch.float32, device=x.device)
            scratch = _bytes(lib.pope_gcn_conv_forward_scratch_size(n, adj.nnz, c_in, c_out), x.device)
            check(lib.pope_gcn_conv_forward(ptr(adj.rowptr), ptr(adj.col), n, adj.nnz, ptr(dinv), self_weight, ptr(x), c_in, ptr(w), ptr(b), c_out,
                                            ptr(out), ptr(scratch), scratch.numel(), _stream()))
        ctx.save_for_backward(x, w, *(() if dinv is None else (dinv,)))
        ctx.adj, ctx.self_weight, ctx.has_bias, ctx.has_dinv = adj, self_weight, b is not None, dinv is not None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib, adj = _lib.load(), ctx.adj
        x, w, *rest = ctx.saved_tensors
        dinv = rest[0] if ctx.has_dinv else None
        g = grad_out.contiguous().float()
        n, (c_in, c_out) = adj.num_nodes, w.shape
        with on_device(x.device):
            grad_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            grad_w = torch.empty_like(w)
            grad_b = torch.empty(c_out, dtype=torch.float32, device=x.device) if ctx.has_bias else None
            scratch = _bytes(lib.pope_gcn_conv_backward_scratch_size(n, adj.nnz, c_in, c_out), x.device)
            check(lib.pope_gcn_conv_backward(ptr(adj.rowptr_t), ptr(adj.col_t), n, adj.nnz, ptr(dinv), ctx.self_weight, ptr(x), c_in, ptr(w), c_out,
                                             ptr(g), ptr(grad_x), ptr(grad_w), ptr(grad_b), ptr(scratch), scratch.numel(), _stream()))
        return grad_x, grad_w, grad_b, None, None, None


class GCNConv(nn.Module):
    """``conv(x, adj)`` over the whole graph, ``adj`` a :class:`GraphAdj`: PyG 1.7.0's ``GCNConv`` [3p, parity unpinned].

    ``normalize=True``: ``f = 2 if improved else 1``; with ``add_self_loops`` the self-loop slots of the graph are skipped and every node
    gets one self term of weight ``f`` (``fill_diag``: the diagonal is replaced, not added to); the edge weight is
    ``dinv_i dinv_j`` with ``deg_i`` the counted slots of row i plus ``f``.  With ``add_self_loops=False`` there is no self term and
    self-loop slots are ordinary edges.  ``normalize=False``: a plain sum over all slots, no self term.  ``cached`` is accepted and changes
    nothing: the normalisation lives in the :class:`GraphAdj`."""

    def __init__(self, in_channels: int, out_channels: int, improved: bool = False, cached: bool = False, add_self_loops: bool = True,
                 normalize: bool = True, bias: bool = True):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.improved, self.cached, self.add_self_loops, self.normalize = bool(improved), bool(cached), bool(add_self_loops), bool(normalize)
        self.weight = nn.Parameter(torch.empty(self.in_channels, self.out_channels))
        self.bias = nn.Parameter(torch.empty(self.out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.in_channels + self.out_channels))          # glorot
        nn.init.uniform_(self.weight, -a, a)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x: torch.Tensor, adj: GraphAdj) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError("GCNConv runs on the GPU only (no CPU fallback)")
        if self.normalize:
            return _GcnConvFn.apply(x, self.weight, self.bias, adj, adj.dinv(self.improved, self.add_self_loops),
                                    adj.self_weight(self.improved, self.add_self_loops))
        return _GcnConvFn.apply(x, self.weight, self.bias, adj, None, 0.0)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}"


class GCN(nn.Module):
    """``num_layers`` GCNConv layers over the whole graph: ``dropout -> conv -> relu`` per layer, the last conv without the ReLU.  Dropout
    and ReLU are torch's own ops."""

    def __init__(self, in_channels: int, hidden_channels: int, out_channels: int, num_layers: int = 2, dropout: float = 0.5, **conv_kwargs):
        super().__init__()
        if num_layers < 1:
            raise ValueError("GCN: num_layers must be at least 1")
        widths = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        self.convs = nn.ModuleList(GCNConv(widths[i], widths[i + 1], **conv_kwargs) for i in range(num_layers))
        self.dropout = float(dropout)

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def forward(self, x: torch.Tensor, adj: GraphAdj) -> torch.Tensor:
        for i, conv in enumerate(self.convs):
            x = F.dropout(x, p=self.dropout, training=self.training)
            x = conv(x, adj)
            if i < len(self.convs) - 1:
                x = x.relu()
        return x
