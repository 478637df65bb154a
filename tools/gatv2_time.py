#!/usr/bin/env python3
"""Time the GATv2 path (csrc/gatv2.h, graphpope_amd/gatv2.py) beside the same layer in stock torch ops (index_select twice, an
[nnz, H, C] leaky, the att reduction, scatter_reduce amax, exp, index_add_, torch's autograd for backward), beside pope_gat_propagate and
beside GATConv, on the Flickr-shaped (N = 89 250, nnz = 899 756) and the PubMed-shaped synthetic graphs, in this one process on one GPU.
Per head shape H x C of 8 x 32, 1 x 256 and 1 x 7, at 756 input channels:

    scores           pope_gatv2_scores alone (e, e_self) on buffers allocated once
    attention        pope_gatv2_attention (scores + edge softmax)
    conv_forward     pope_gatv2_conv_forward at 756 -> H x C
    conv_backward    pope_gatv2_conv_backward (with grad_x and every bias gradient)
    torch_<the same> the stock-torch form of each
    gat_propagate    pope_gat_propagate over the same hl behind that alpha (concat, bias): the bytes the score pass moves
    gat_conv_forward / gat_conv_backward   GATConv at the same shape (pope_gat_conv_*)
and once per graph:
    train_step       one full-batch training step of GATv2(756, 256, 7, heads=8): forward at dropout 0.5, the loss on the training rows
                     (sage.cross_entropy), backward, optim.Adam(max_grad_norm=0.5); torch_train_step: the stock-torch form with
                     F.cross_entropy, clip_grad_norm_ and torch.optim.Adam

The time between two HIP events around a block of --steps calls, divided by the calls; --reps blocks per form (five), the forms taken in
turns so that drift of the machine lands on all alike; median [min - max] per form.  The two forms' results are compared first (scores
and attention: per destination, every slot's output in the sums; the backward pass: both against the float64 form of the same ops under the library's LeakyReLU pattern, the library's error at most 4 x the stock float32 form's).  Prints one JSON object; --out FILE also writes it there
(profiles/gatv2_times.json).  The run ends itself after --time-limit seconds; run it under `timeout` too."""
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
from graphpope_amd import _lib, engine, gat, gatv2, optim, sage, synth  # noqa: E402

C_IN, HIDDEN, CLASSES, HEADS = 756, 256, 7, 8
SHAPES = ((8, 32), (1, 256), (1, 7))
GRAPHS = {"flickr": synth.flickr_like, "pubmed": synth.pubmed_like}
SLOPE = 0.2
GRADS = ("x", "lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "att", "bias")


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


def torch_scores(hl, hr, att, src, dst, pattern=None):
    """e [E, H] over the term list (self-loop slots dropped, one self term per node appended), stock torch ops.  pattern: bool [E, H, C],
    the side of the LeakyReLU every element takes (the comparison of the backward passes: one element of z within rounding of 0 that
    falls on the other side moves the heavily cancelling gradients by 1e-3 of their largest entry)."""
    z = hl.index_select(0, src) + hr.index_select(0, dst)
    return ((F.leaky_relu(z, SLOPE) if pattern is None else torch.where(pattern, z, SLOPE * z)) * att).sum(-1)


def torch_attention(hl, hr, att, src, dst, n, pattern=None):
    e = torch_scores(hl, hr, att, src, dst, pattern)
    H = e.shape[1]
    top = torch.full((n, H), float("-inf"), device=e.device, dtype=e.dtype).scatter_reduce(0, dst[:, None].expand(-1, H), e.detach(), "amax", include_self=True)
    ex = torch.exp(e - top.index_select(0, dst))
    s = torch.zeros((n, H), device=e.device, dtype=e.dtype).index_add_(0, dst, ex)
    return ex / s.index_select(0, dst)


def torch_conv(x, wl, bl, wr, br, att, b, src, dst, H, C, pattern=None):
    n = x.shape[0]
    hl, hr = F.linear(x, wl, bl).view(n, H, C), F.linear(x, wr, br).view(n, H, C)
    alpha = torch_attention(hl, hr, att, src, dst, n, pattern)
    return torch.zeros_like(hl).index_add_(0, dst, alpha[:, :, None] * hl.index_select(0, src)).reshape(n, H * C) + b


class TorchGatV2(torch.nn.Module):
    def __init__(self, world):
        super().__init__()
        self.w = world
        self.params = torch.nn.ParameterList(torch.nn.Parameter(p.detach().clone()) for c in world.model.convs
                                             for p in (c.lin_l.weight, c.lin_l.bias, c.lin_r.weight, c.lin_r.bias, c.att, c.bias))

    def forward(self, x, p):
        for i, (H, C) in enumerate(((HEADS, HIDDEN // HEADS), (1, CLASSES))):
            x = torch_conv(F.dropout(x, p, self.training), *self.params[6 * i:6 * i + 6], self.w.src, self.w.dst, H, C)
            if i == 0:
                x = F.elu(x)
        return x


class World:
    def __init__(self, name, dev):
        ei, n = GRAPHS[name]()
        self.name, self.n, self.dev, self.lib = name, n, dev, _lib.load()
        ei = torch.as_tensor(ei).to(dev)
        self.adj = gatv2.GraphAdj(ei, n)
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
            self.shape[H, C] = {"hl": rnd(n, H * C), "hr": rnd(n, H * C), "att": rnd(1, H, C), "att_r": rnd(1, H, C), "b": rnd(H * C),
                                "g": rnd(n, H * C), "wl": (rnd(H * C, C_IN) / 10).contiguous(), "wr": (rnd(H * C, C_IN) / 10).contiguous(),
                                "bl": rnd(H * C) / 10, "br": rnd(H * C) / 10}
        torch.manual_seed(0)
        self.model = gatv2.GATv2(C_IN, HIDDEN, CLASSES, num_layers=2, heads=HEADS, dropout=0.5).to(dev).train()
        self.opt = optim.Adam(self.model.parameters(), lr=1e-3, max_grad_norm=0.5)
        self.tmodel = TorchGatV2(self).to(dev).train()
        self.topt = torch.optim.Adam(self.tmodel.parameters(), lr=1e-3)
        self._calls = {}

    def _raw(self, key, build):
        if key not in self._calls:
            self._calls[key] = build()
        return self._calls[key]

    def _buffers(self, H, C):
        def build():
            f = lambda *s: torch.empty(s, dtype=torch.float32, device=self.dev)                          # noqa: E731
            return {"hl": f(self.n, H * C), "hr": f(self.n, H * C), "e": f(self.nnz, H), "e_self": f(self.n, H), "alpha": f(self.nnz, H),
                    "alpha_self": f(self.n, H), "out": f(self.n, H * C), "h": f(self.n, H * C), "a_src": f(self.n, H), "a_dst": f(self.n, H),
                    "galpha": f(self.nnz, H), "galpha_self": f(self.n, H)}
        return self._raw(("buffers", H, C), build)

    def _scratch(self, key, query, *args):
        return self._raw(("scratch", key) + args, lambda: torch.empty(max(query(*args), 256), dtype=torch.uint8, device=self.dev))

    # ---- the library's
    def scores(self, H, C):
        s, o, p, a = self.shape[H, C], self._buffers(H, C), _lib.ptr, self.adj
        _lib.check(self.lib.pope_gatv2_scores(p(a.rowptr), p(a.col), self.n, self.nnz, p(s["hl"]), p(s["hr"]), H, C, p(s["att"]), SLOPE, 1, p(o["e"]),
                                              p(o["e_self"]), sage._stream()))
        return o["e"], o["e_self"]

    def attention(self, H, C):
        s, o, p, a = self.shape[H, C], self._buffers(H, C), _lib.ptr, self.adj
        _lib.check(self.lib.pope_gatv2_attention(p(a.rowptr), p(a.col), self.n, self.nnz, p(s["hl"]), p(s["hr"]), H, C, p(s["att"]), SLOPE, 1,
                                                 p(o["e"]), p(o["e_self"]), p(o["alpha"]), p(o["alpha_self"]), sage._stream()))
        return o["alpha"], o["alpha_self"]

    def gat_propagate(self, H, C):
        """Behind attention of the same shape (its alpha is in the buffers)."""
        s, o, p, a = self.shape[H, C], self._buffers(H, C), _lib.ptr, self.adj
        scratch = self._scratch("propagate", self.lib.pope_gat_propagate_scratch_size, self.n, self.nnz, H, C, 1)
        _lib.check(self.lib.pope_gat_propagate(p(a.rowptr), p(a.col), self.n, self.nnz, p(o["alpha"]), p(o["alpha_self"]), p(s["hl"]), H, C, 1,
                                               p(s["b"]), p(o["out"]), p(scratch), scratch.numel(), sage._stream()))
        return o["out"]

    def conv_forward(self, H, C):
        s, o, p, a = self.shape[H, C], self._buffers(H, C), _lib.ptr, self.adj
        scratch = self._scratch("forward", self.lib.pope_gatv2_conv_forward_scratch_size, self.n, self.nnz, C_IN, H, C, 1)
        _lib.check(self.lib.pope_gatv2_conv_forward(p(a.rowptr), p(a.col), self.n, self.nnz, p(self.x), C_IN, p(s["wl"]), p(s["bl"]), p(s["wr"]),
                                                    p(s["br"]), p(s["att"]), p(s["b"]), H, C, 1, SLOPE, 1, p(o["hl"]), p(o["hr"]), p(o["alpha"]),
                                                    p(o["alpha_self"]), p(o["out"]), p(scratch), scratch.numel(), sage._stream()))
        return o["out"]

    def conv_backward(self, H, C):
        """Behind conv_forward of the same shape (its hl, hr and alpha are in the buffers)."""
        s, o, p, a = self.shape[H, C], self._buffers(H, C), _lib.ptr, self.adj
        grads = self._raw(("grads", H, C), lambda: tuple(torch.empty_like(t) for t in (self.x, s["wl"], s["bl"], s["wr"], s["br"], s["att"], s["b"])))
        scratch = self._scratch("backward", self.lib.pope_gatv2_conv_backward_scratch_size, self.n, self.nnz, C_IN, H, C, 1)
        _lib.check(self.lib.pope_gatv2_conv_backward(p(a.rowptr), p(a.col), p(a.rowptr_t), p(a.col_t), p(a.slot_map), self.n, self.nnz, p(self.x),
                                                     C_IN, p(s["wl"]), p(s["wr"]), p(s["att"]), H, C, 1, SLOPE, 1, p(o["hl"]), p(o["hr"]),
                                                     p(o["alpha"]), p(o["alpha_self"]), p(s["g"]), *(p(t) for t in grads), p(scratch),
                                                     scratch.numel(), sage._stream()))
        return grads

    def gat_conv_forward(self, H, C):
        s, o, p, a = self.shape[H, C], self._buffers(H, C), _lib.ptr, self.adj
        scratch = self._scratch("gforward", self.lib.pope_gat_conv_forward_scratch_size, self.n, self.nnz, C_IN, H, C, 1)
        _lib.check(self.lib.pope_gat_conv_forward(p(a.rowptr), p(a.col), self.n, self.nnz, p(self.x), C_IN, p(s["wl"]), p(s["att"]), p(s["att_r"]),
                                                  p(s["b"]), H, C, 1, SLOPE, 1, p(o["h"]), p(o["a_src"]), p(o["a_dst"]), p(o["galpha"]),
                                                  p(o["galpha_self"]), p(o["out"]), p(scratch), scratch.numel(), sage._stream()))
        return o["out"]

    def gat_conv_backward(self, H, C):
        s, o, p, a = self.shape[H, C], self._buffers(H, C), _lib.ptr, self.adj
        grads = self._raw(("ggrads", H, C), lambda: tuple(torch.empty_like(t) for t in (self.x, s["wl"], s["att"], s["att_r"], s["b"])))
        scratch = self._scratch("gbackward", self.lib.pope_gat_conv_backward_scratch_size, self.n, self.nnz, C_IN, H, C, 1)
        _lib.check(self.lib.pope_gat_conv_backward(p(a.rowptr), p(a.col), p(a.rowptr_t), p(a.col_t), p(a.slot_map), self.n, self.nnz, p(self.x), C_IN,
                                                   p(s["wl"]), p(s["att"]), p(s["att_r"]), H, C, 1, SLOPE, 1, p(o["h"]), p(o["a_src"]), p(o["a_dst"]),
                                                   p(o["galpha"]), p(o["galpha_self"]), p(s["g"]), *(p(t) for t in grads), p(scratch),
                                                   scratch.numel(), sage._stream()))
        return grads

    def train_step(self):
        for p in self.model.parameters():
            p.grad = None
        loss = sage.cross_entropy(self.model(self.x, self.adj).index_select(0, self.train_rows), self.y_train)
        loss.backward()
        self.opt.step()
        return loss

    def per_destination(self, slots, own=None):
        """[n, 2 H] in float64: per destination the sum and the sum of squares of a per-term quantity -- given per slot of the CSR by
        destination with the self terms apart (the library's: a slot that is no term holds 0), or per term of the term list."""
        if own is None:
            rows, x = self.dst, slots.double()
        else:
            rows = torch.repeat_interleave(torch.arange(self.n, device=self.dev), (self.adj.rowptr[1:self.n + 1] - self.adj.rowptr[:self.n]).long())
            rows, x = torch.cat([rows, torch.arange(self.n, device=self.dev)]), torch.cat([slots[:self.nnz], own]).double()
        return torch.zeros((self.n, 2 * x.shape[1]), dtype=torch.float64, device=self.dev).index_add_(0, rows, torch.cat([x, x * x], 1))

    # ---- the stock-torch forms
    def torch_scores(self, H, C):
        s = self.shape[H, C]
        return torch_scores(s["hl"].view(self.n, H, C), s["hr"].view(self.n, H, C), s["att"], self.src, self.dst)

    def torch_attention(self, H, C):
        s = self.shape[H, C]
        return torch_attention(s["hl"].view(self.n, H, C), s["hr"].view(self.n, H, C), s["att"], self.src, self.dst, self.n)

    def _leaves(self, H, C):
        s = self.shape[H, C]
        return [self.x] + [s[k] for k in ("wl", "bl", "wr", "br", "att", "b")]

    def torch_conv_forward(self, H, C):
        return torch_conv(*self._leaves(H, C), self.src, self.dst, H, C)

    def device_pattern(self, H, C):
        """Behind conv_forward of the same shape: hl[j] + hr[i] > 0 of every term, summed in float32 from the library's own hl and hr."""
        o = self._buffers(H, C)
        return (o["hl"].index_select(0, self.src) + o["hr"].index_select(0, self.dst)).view(-1, H, C) > 0

    def torch_conv_backward(self, H, C, dtype=torch.float32, pattern=None):
        leaves = [t.detach().to(dtype).requires_grad_(True) for t in self._leaves(H, C)]
        out = torch_conv(*leaves, self.src, self.dst, H, C, pattern)
        return torch.autograd.grad(out, leaves, self.shape[H, C]["g"].to(dtype))

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
            b = ctypes.create_string_buffer(1536)
            _lib.check(self.lib.pope_gatv2_kernel_name(self.n, self.nnz, C_IN, H, C, 1, 0, backward, 1, cus, 0, b, 1536))
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

    res = {"shape": {"in_channels": C_IN, "head_shapes": ["%dx%d" % s for s in SHAPES], "model": "GATv2(756, 256, 7, heads=8), 2 layers, dropout 0.5"},
           "calls_per_block": args.steps, "warmup_calls": args.warmup, "reps": args.reps, "unit": "us per call, HIP events around a block",
           "device": torch.cuda.get_device_name(0), "compute_units": cus, "graphs": {}}
    for name in args.graphs.split(","):
        w = World(name, dev)
        forms, agreement, launches, backward_vs_float64 = {"train_step": w.train_step, "torch_train_step": w.torch_train_step}, {}, {}, {}
        for H, C in SHAPES:
            tag = "%dx%d" % (H, C)
            # (in this order: gat_propagate reads attention's alpha, conv_backward what conv_forward left)
            for k in ("scores", "attention", "gat_propagate", "conv_forward", "conv_backward", "gat_conv_forward", "gat_conv_backward"):
                forms[k + "_" + tag] = lambda k=k, H=H, C=C: getattr(w, k)(H, C)
                if not k.startswith("gat_"):
                    forms["torch_" + k + "_" + tag] = lambda k=k, H=H, C=C: getattr(w, "torch_" + k)(H, C)
            # every slot's output, per destination: the term list and the CSR hold a row's terms in different orders, so the sums and the
            # sums of squares over each destination's terms (slots and self term) are compared, and the self terms one by one
            e, e_self = w.scores(H, C)
            te = w.torch_scores(H, C)
            agreement["scores_" + tag] = max(rel_err(e_self, te[-w.n:]), rel_err(w.per_destination(e, e_self), w.per_destination(te)))
            alpha, alpha_self = w.attention(H, C)
            ta = w.torch_attention(H, C)
            agreement["attention_" + tag] = max(rel_err(alpha_self, ta[-w.n:]), rel_err(w.per_destination(alpha, alpha_self), w.per_destination(ta)))
            del te, ta
            agreement["conv_forward_" + tag] = rel_err(w.conv_forward(H, C), w.torch_conv_forward(H, C))
            # the gradients cancel heavily (the de of a row sum to 0): both float32 forms are held against the float64 form of the same ops,
            # all three under the library's LeakyReLU pattern
            pattern = w.device_pattern(H, C)
            ref = w.torch_conv_backward(H, C, torch.float64, pattern)
            mine = {k: rel_err(a, b) for k, a, b in zip(GRADS, w.conv_backward(H, C), ref)}
            stock = {k: rel_err(a, b) for k, a, b in zip(GRADS, w.torch_conv_backward(H, C, torch.float32, pattern), ref)}
            backward_vs_float64[tag] = {"library": mine, "torch_float32": stock}
            del ref, pattern
            w.attention(H, C)
            launches[tag] = w.kernel_names(cus, H, C)
        print(json.dumps({"graph": name, "agreement": agreement, "backward_vs_float64": backward_vs_float64}), file=sys.stderr, flush=True)
        assert max(agreement.values()) < 1e-3, agreement
        for tag, both in backward_vs_float64.items():
            for k in GRADS:
                assert both["library"][k] <= 4.0 * max(both["torch_float32"][k], 2.0 ** -23), (tag, k, both)
        for fn in forms.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, fn in forms.items():
                times[k].append(events_us(fn, args.steps))
        out = {"nodes": w.n, "slots": w.nnz, "max_relative_difference": agreement, "backward_error_against_float64": backward_vs_float64,
               "launch_lists": launches,
               "forms": {k: stats(ts) for k, ts in times.items()}}
        for H, C in SHAPES:
            tag = "%dx%d" % (H, C)
            out["scores_%s_over_gat_propagate" % tag] = out["forms"]["scores_" + tag]["median"] / out["forms"]["gat_propagate_" + tag]["median"]
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
