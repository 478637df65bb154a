#!/usr/bin/env python3
"""Time the GAT path (csrc/gat.h, graphpope_amd/gat.py) beside the same computation in stock torch ops (index_select, scatter_reduce amax,
exp, index_add_) and beside pope_gcn_propagate at C = 256, on the Flickr-shaped (N = 89 250, nnz = 899 756) and the PubMed-shaped
synthetic graphs, in this one process on one GPU.  Per head shape H x C of 8 x 32, 1 x 256 and 1 x 7:

    attention        pope_gat_attention alone (scores + edge softmax) on buffers allocated once
    propagate        pope_gat_propagate alone behind that alpha (concat, bias)
    conv_forward     pope_gat_conv_forward at 756 -> H x C
    conv_backward    pope_gat_conv_backward (with grad_x and grad_bias)
    torch_<the same> the stock-torch form of each
and once per graph:
    gcn_propagate_c256   pope_gcn_propagate at C = 256 (dinv, f = 1, bias): the same rows moved, no per-edge weights
    train_step           one full-batch training step of GAT(756, 256, 7, heads=8): forward at dropout 0.5, the loss on the training rows
                         (sage.cross_entropy), backward, optim.Adam(max_grad_norm=0.5); torch_train_step: the stock-torch form with
                         F.cross_entropy, clip_grad_norm_ and torch.optim.Adam

The time between two HIP events around a block of --steps calls, divided by the calls; --reps blocks per form (five), the forms taken in
turns so that drift of the machine lands on all alike; median [min - max] per form.  The two forms' results are compared first.  Prints one
JSON object; --out FILE also writes it there (profiles/gat_times.json).  The run ends itself after --time-limit seconds; run it under
`timeout` too."""
import argparse
import ctypes
import faulthandler
import gc
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphpope_amd import _lib, engine, gat, optim, sage, synth  # noqa: E402

C_IN, HIDDEN, CLASSES, HEADS = 756, 256, 7, 8
SHAPES = ((8, 32), (1, 256), (1, 7))
GRAPHS = {"flickr": synth.flickr_like, "pubmed": synth.pubmed_like}
SLOPE = 0.2


def events_us(fn, k):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(k):
        fn()
    t1.record()
    t1.synchronize()
    return 1e3 * t0.elapsed_time(t1) / k


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def torch_attention(h, att_l, att_r, src, dst, n):
    """(alpha [E, H]) over the term list (self-loop slots dropped, one self term per node appended), stock torch ops."""
    H = h.shape[1]
    e = F.leaky_relu((h * att_l).sum(-1).index_select(0, src) + (h * att_r).sum(-1).index_select(0, dst), SLOPE)
    top = torch.full((n, H), float("-inf"), device=h.device).scatter_reduce(0, dst[:, None].expand(-1, H), e.detach(), "amax", include_self=True)
    ex = torch.exp(e - top.index_select(0, dst))
    s = torch.zeros((n, H), device=h.device).index_add_(0, dst, ex)
    return ex / s.index_select(0, dst)


def torch_propagate(h, alpha, src, dst):
    return torch.zeros_like(h).index_add_(0, dst, alpha[:, :, None] * h.index_select(0, src))


def torch_conv(x, w, att_l, att_r, b, src, dst, H, C):
    h = (x @ w.t()).view(x.shape[0], H, C)
    return torch_propagate(h, torch_attention(h, att_l, att_r, src, dst, x.shape[0]), src, dst).reshape(x.shape[0], H * C) + b


class TorchGat(torch.nn.Module):
    def __init__(self, world):
        super().__init__()
        self.w = world
        self.params = torch.nn.ParameterList(torch.nn.Parameter(p.detach().clone()) for c in world.model.convs
                                             for p in (c.lin_l.weight, c.att_l, c.att_r, c.bias))

    def forward(self, x, p):
        for i, (H, C) in enumerate(((HEADS, HIDDEN // HEADS), (1, CLASSES))):
            w, al, ar, b = self.params[4 * i:4 * i + 4]
            x = torch_conv(F.dropout(x, p, self.training), w, al, ar, b, self.w.src, self.w.dst, H, C)
            if i == 0:
                x = F.elu(x)
        return x


class World:
    def __init__(self, name, dev):
        ei, n = GRAPHS[name]()
        self.name, self.n, self.dev, self.lib = name, n, dev, _lib.load()
        ei = torch.as_tensor(ei).to(dev)
        self.adj = gat.GraphAdj(ei, n)
        self.nnz = self.adj.nnz
        self.adj.slot_map                                               # built once, outside the timed calls
        keep = ei[0] != ei[1]
        loops = torch.arange(n, device=dev)
        self.src, self.dst = torch.cat([ei[0][keep], loops]).contiguous(), torch.cat([ei[1][keep], loops]).contiguous()
        g = torch.Generator().manual_seed(0)
        self.x = torch.rand(n, C_IN, generator=g).to(dev)
        self.y = torch.randint(0, CLASSES, (n,), generator=g).to(dev)
        self.train_rows = torch.nonzero(torch.rand(n, generator=g) < 0.5).flatten().to(dev)
        self.y_train = self.y.index_select(0, self.train_rows)
        self.shape = {}
        for H, C in SHAPES:
            rnd = lambda *s: (torch.rand(*s, generator=g) - 0.5).to(dev)                                  # noqa: E731
            self.shape[H, C] = {"h": rnd(n, H * C), "att_l": rnd(1, H, C), "att_r": rnd(1, H, C), "b": rnd(H * C), "g": rnd(n, H * C),
                                "w": (rnd(H * C, C_IN) / 10).contiguous()}
        self.h256, self.b256 = self.shape[1, 256]["h"], self.shape[1, 256]["b"]
        torch.manual_seed(0)
        self.model = gat.GAT(C_IN, HIDDEN, CLASSES, num_layers=2, heads=HEADS, dropout=0.5).to(dev).train()
        self.opt = optim.Adam(self.model.parameters(), lr=1e-3, max_grad_norm=0.5)
        self.tmodel = TorchGat(self).to(dev).train()
        self.topt = torch.optim.Adam(self.tmodel.parameters(), lr=1e-3)
        self._calls = {}

    def _raw(self, key, build):
        if key not in self._calls:
            self._calls[key] = build()
        return self._calls[key]

    def _buffers(self, H, C):
        def build():
            f = lambda *s: torch.empty(s, dtype=torch.float32, device=self.dev)                          # noqa: E731
            return {"h": f(self.n, H * C), "a_src": f(self.n, H), "a_dst": f(self.n, H), "alpha": f(self.nnz, H), "alpha_self": f(self.n, H),
                    "out": f(self.n, H * C)}
        return self._raw(("buffers", H, C), build)

    def _scratch(self, key, query, *args):
        return self._raw(("scratch", key) + args, lambda: torch.empty(max(query(*args), 256), dtype=torch.uint8, device=self.dev))

    # ---- the library's
    def attention(self, H, C):
        s, o, p, a = self.shape[H, C], self._buffers(H, C), _lib.ptr, self.adj
        _lib.check(self.lib.pope_gat_attention(p(a.rowptr), p(a.col), self.n, self.nnz, p(s["h"]), H, C, p(s["att_l"]), p(s["att_r"]), SLOPE, 1,
                                               p(o["a_src"]), p(o["a_dst"]), p(o["alpha"]), p(o["alpha_self"]), sage._stream()))
        return o["alpha"], o["alpha_self"]

    def propagate(self, H, C):
        s, o, p, a = self.shape[H, C], self._buffers(H, C), _lib.ptr, self.adj
        scratch = self._scratch("propagate", self.lib.pope_gat_propagate_scratch_size, self.n, self.nnz, H, C, 1)
        _lib.check(self.lib.pope_gat_propagate(p(a.rowptr), p(a.col), self.n, self.nnz, p(o["alpha"]), p(o["alpha_self"]), p(s["h"]), H, C, 1,
                                               p(s["b"]), p(o["out"]), p(scratch), scratch.numel(), sage._stream()))
        return o["out"]

    def conv_forward(self, H, C):
        s, o, p, a = self.shape[H, C], self._buffers(H, C), _lib.ptr, self.adj
        scratch = self._scratch("forward", self.lib.pope_gat_conv_forward_scratch_size, self.n, self.nnz, C_IN, H, C, 1)
        _lib.check(self.lib.pope_gat_conv_forward(p(a.rowptr), p(a.col), self.n, self.nnz, p(self.x), C_IN, p(s["w"]), p(s["att_l"]), p(s["att_r"]),
                                                  p(s["b"]), H, C, 1, SLOPE, 1, p(o["h"]), p(o["a_src"]), p(o["a_dst"]), p(o["alpha"]),
                                                  p(o["alpha_self"]), p(o["out"]), p(scratch), scratch.numel(), sage._stream()))
        return o["out"]

    def conv_backward(self, H, C):
        """Behind conv_forward of the same shape (its h, scores and alpha are in the buffers)."""
        s, o, p, a = self.shape[H, C], self._buffers(H, C), _lib.ptr, self.adj
        grads = self._raw(("grads", H, C), lambda: (torch.empty_like(self.x), torch.empty_like(s["w"]), torch.empty_like(s["att_l"]),
                                                     torch.empty_like(s["att_r"]), torch.empty_like(s["b"])))
        scratch = self._scratch("backward", self.lib.pope_gat_conv_backward_scratch_size, self.n, self.nnz, C_IN, H, C, 1)
        _lib.check(self.lib.pope_gat_conv_backward(p(a.rowptr), p(a.col), p(a.rowptr_t), p(a.col_t), p(a.slot_map), self.n, self.nnz, p(self.x), C_IN,
                                                   p(s["w"]), p(s["att_l"]), p(s["att_r"]), H, C, 1, SLOPE, 1, p(o["h"]), p(o["a_src"]), p(o["a_dst"]),
                                                   p(o["alpha"]), p(o["alpha_self"]), p(s["g"]), *(p(t) for t in grads), p(scratch), scratch.numel(),
                                                   sage._stream()))
        return grads

    def gcn_propagate_c256(self):
        p, a = _lib.ptr, self.adj
        out = self._raw("gcn_out", lambda: torch.empty_like(self.h256))
        scratch = self._scratch("gcn", self.lib.pope_gcn_propagate_scratch_size, self.n, self.nnz, 256)
        _lib.check(self.lib.pope_gcn_propagate(p(a.rowptr), p(a.col), self.n, self.nnz, p(a.dinv()), 1.0, p(self.h256), 256, p(self.b256), p(out),
                                               p(scratch), scratch.numel(), sage._stream()))
        return out

    def train_step(self):
        for p in self.model.parameters():
            p.grad = None
        loss = sage.cross_entropy(self.model(self.x, self.adj).index_select(0, self.train_rows), self.y_train)
        loss.backward()
        self.opt.step()
        return loss

    # ---- the stock-torch forms
    def torch_attention(self, H, C):
        s = self.shape[H, C]
        return torch_attention(s["h"].view(self.n, H, C), s["att_l"], s["att_r"], self.src, self.dst, self.n)

    def torch_propagate(self, H, C):
        s = self.shape[H, C]
        alpha = self._raw(("talpha", H, C), lambda: self.torch_attention(H, C))
        return torch_propagate(s["h"].view(self.n, H, C), alpha, self.src, self.dst).reshape(self.n, H * C) + s["b"]

    def torch_conv_forward(self, H, C):
        s = self.shape[H, C]
        return torch_conv(self.x, s["w"], s["att_l"], s["att_r"], s["b"], self.src, self.dst, H, C)

    def torch_conv_backward(self, H, C):
        s = self.shape[H, C]
        leaves = [t.detach().requires_grad_(True) for t in (self.x, s["w"], s["att_l"], s["att_r"], s["b"])]
        out = torch_conv(*leaves, self.src, self.dst, H, C)
        return torch.autograd.grad(out, leaves, s["g"])

    def torch_train_step(self):
        self.topt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(self.tmodel(self.x, 0.5).index_select(0, self.train_rows), self.y_train)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.tmodel.parameters(), 0.5)
        self.topt.step()
        return loss

    def kernel_names(self, cus, H, C):
        names = {}
        for key, backward in (("conv_forward", 0), ("conv_backward", 1)):
            b = ctypes.create_string_buffer(768)
            _lib.check(self.lib.pope_gat_kernel_name(self.n, self.nnz, C_IN, H, C, 1, backward, 1, cus, 0, b, 768))
            names[key] = b.value.decode()
        return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--graphs", default="flickr,pubmed")
    ap.add_argument("--time-limit", type=int, default=420, help="seconds after which the run ends itself")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.time_limit, exit=True)
    dev = engine.require_gpu()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def stats(ts):
        return {"median": float(np.median(ts)), "min": min(ts), "max": max(ts), "all": ts}

    res = {"shape": {"in_channels": C_IN, "head_shapes": ["%dx%d" % s for s in SHAPES], "model": "GAT(756, 256, 7, heads=8), 2 layers, dropout 0.5"},
           "calls_per_block": args.steps, "warmup_calls": args.warmup, "reps": args.reps, "unit": "us per call, HIP events around a block",
           "device": torch.cuda.get_device_name(0), "compute_units": cus, "graphs": {}}
    for name in args.graphs.split(","):
        w = World(name, dev)
        forms, agreement, launches = {"gcn_propagate_c256": w.gcn_propagate_c256, "train_step": w.train_step, "torch_train_step": w.torch_train_step}, {}, {}
        for H, C in SHAPES:
            tag = "%dx%d" % (H, C)
            for k in ("attention", "propagate", "conv_forward", "conv_backward"):          # (in this order: each reads what the one before left)
                forms[k + "_" + tag] = lambda k=k, H=H, C=C: getattr(w, k)(H, C)
                forms["torch_" + k + "_" + tag] = lambda k=k, H=H, C=C: getattr(w, "torch_" + k)(H, C)
            alpha, alpha_self = w.attention(H, C)
            talpha = w.torch_attention(H, C)
            agreement["attention_" + tag] = rel_err(alpha_self, talpha[-w.n:])
            agreement["conv_forward_" + tag] = rel_err(w.conv_forward(H, C), w.torch_conv_forward(H, C))
            agreement["conv_backward_" + tag] = max(rel_err(a, b) for a, b in zip(w.conv_backward(H, C), w.torch_conv_backward(H, C)))
            w.attention(H, C)                                                              # the propagate's alpha: of the given h again
            launches[tag] = w.kernel_names(cus, H, C)
        assert max(agreement.values()) < 1e-3, agreement
        for fn in forms.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, fn in forms.items():
                times[k].append(events_us(fn, args.steps))
        out = {"nodes": w.n, "slots": w.nnz, "max_relative_difference": agreement, "launch_lists": launches,
               "forms": {k: stats(ts) for k, ts in times.items()}}
        out["propagate_8x32_over_gcn_propagate_c256"] = out["forms"]["propagate_8x32"]["median"] / out["forms"]["gcn_propagate_c256"]["median"]
        out["propagate_1x256_over_gcn_propagate_c256"] = out["forms"]["propagate_1x256"]["median"] / out["forms"]["gcn_propagate_c256"]["median"]
        res["graphs"][name] = out
        del w, forms, fn
        gc.collect()
        torch.cuda.empty_cache()
    faulthandler.cancel_dump_traceback_later()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
