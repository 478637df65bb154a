#!/usr/bin/env python3
"""Time the GCN path (csrc/gcn.h, graphpope_amd/gcn.py) beside the same computation in stock torch ops (index_select + index_add_ +
matmul) on the Flickr-shaped (N = 89 250, nnz = 899 756) and the PubMed-shaped synthetic graphs, in this one process on one GPU:

    propagate_c256 / propagate_c7        pope_gcn_propagate alone (dinv, f = 1, bias) on buffers allocated once
    conv_forward / conv_backward         pope_gcn_conv_forward / _backward at 756 -> 256 (backward: with grad_x and grad_bias)
    train_step                           one full-batch training step of GCN(756, 256, 7): forward at dropout 0.5, the loss on the
                                         training rows (sage.cross_entropy), backward, optim.Adam(max_grad_norm=0.5)
    torch_<the same>                     the stock-torch form of each; the step with F.cross_entropy, clip_grad_norm_ and torch.optim.Adam

The time between two HIP events around a block of --steps calls, divided by the calls; --reps blocks per form (five), the forms taken
in turns so that drift of the machine lands on all alike; median [min - max] per form.  The two forms' results are compared first.
For the propagate the achieved bytes/s against nnz C 4 + 2 N C 4 + 8 nnz, and beside it the aggregate of sage_full_layer_forward at the
same width from profiles/full_inference_times.json (a kernel trace there, HIP events here).  Prints one JSON object; --out FILE also writes
it there (profiles/gcn_times.json).  Per-launch times come from a kernel trace, a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 tools/gcn_time.py --trace <graph> <form>
The run ends itself after --time-limit seconds; run it under `timeout` too."""
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
from graphpope_amd import _lib, engine, gcn, optim, sage, synth  # noqa: E402

C_IN, HIDDEN, CLASSES = 756, 256, 7
GRAPHS = {"flickr": synth.flickr_like, "pubmed": synth.pubmed_like}


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


class TorchGcn(torch.nn.Module):
    """GCN(756, 256, 7) in stock torch ops over the edge list."""

    def __init__(self, world):
        super().__init__()
        self.w = world
        self.weights = torch.nn.ParameterList(torch.nn.Parameter(c.weight.detach().clone()) for c in world.model.convs)
        self.biases = torch.nn.ParameterList(torch.nn.Parameter(c.bias.detach().clone()) for c in world.model.convs)

    def forward(self, x, p):
        for i, (w, b) in enumerate(zip(self.weights, self.biases)):
            x = self.w.torch_propagate(F.dropout(x, p, self.training) @ w, False) + b
            if i == 0:
                x = x.relu()
        return x


class World:
    def __init__(self, name, dev):
        ei, n = GRAPHS[name]()
        self.name, self.n, self.dev, self.lib = name, n, dev, _lib.load()
        ei = torch.as_tensor(ei).to(dev)
        self.adj = gcn.GraphAdj(ei, n)
        self.nnz = self.adj.nnz
        self.dinv = self.adj.dinv()
        src, dst = ei[0], ei[1]
        keep = src != dst                                               # the torch form: the diagonal replaced by one self term
        self.src, self.dst = src[keep].contiguous(), dst[keep].contiguous()
        self.edge_w = (self.dinv[self.src] * self.dinv[self.dst])[:, None].contiguous()
        self.own_w = (self.dinv * self.dinv)[:, None].contiguous()
        g = torch.Generator().manual_seed(0)
        self.x = torch.rand(n, C_IN, generator=g).to(dev)
        self.h = {c: torch.rand(n, c, generator=g).to(dev) for c in (HIDDEN, CLASSES)}
        self.b = {c: torch.rand(c, generator=g).to(dev) for c in (HIDDEN, CLASSES)}
        self.g_out = torch.rand(n, HIDDEN, generator=g).to(dev)
        self.y = torch.randint(0, CLASSES, (n,), generator=g).to(dev)
        self.train_rows = torch.nonzero(torch.rand(n, generator=g) < 0.5).flatten().to(dev)
        self.y_train = self.y.index_select(0, self.train_rows)
        torch.manual_seed(0)
        self.model = gcn.GCN(C_IN, HIDDEN, CLASSES, num_layers=2, dropout=0.5).to(dev).train()
        self.opt = optim.Adam(self.model.parameters(), lr=1e-3, max_grad_norm=0.5)
        self.tmodel = TorchGcn(self).to(dev).train()
        self.topt = torch.optim.Adam(self.tmodel.parameters(), lr=1e-3)
        self.weight = self.model.convs[0].weight.detach()
        self.bias0 = self.b[HIDDEN]
        self._calls = {}

    # ---- the stock-torch forms
    def torch_propagate(self, h, transposed):
        src, dst = (self.dst, self.src) if transposed else (self.src, self.dst)
        out = torch.zeros_like(h).index_add_(0, dst, h.index_select(0, src) * self.edge_w)
        return out + self.own_w * h

    def torch_propagate_c256(self):
        return self.torch_propagate(self.h[HIDDEN], False) + self.b[HIDDEN]

    def torch_propagate_c7(self):
        return self.torch_propagate(self.h[CLASSES], False) + self.b[CLASSES]

    def torch_conv_forward(self):
        return self.torch_propagate(self.x @ self.weight, False) + self.bias0

    def torch_conv_backward(self):
        t = self.torch_propagate(self.g_out, True)
        return t @ self.weight.T, self.x.T @ t, self.g_out.sum(0)

    def torch_train_step(self):
        self.topt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(self.tmodel(self.x, 0.5).index_select(0, self.train_rows), self.y_train)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.tmodel.parameters(), 0.5)
        self.topt.step()
        return loss

    # ---- the library's
    def _raw(self, key, build):
        if key not in self._calls:
            self._calls[key] = build()
        return self._calls[key]()

    def _propagate(self, c):
        def build():
            out = torch.empty((self.n, c), dtype=torch.float32, device=self.dev)
            nbytes = self.lib.pope_gcn_propagate_scratch_size(self.n, self.nnz, c)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            p, a = _lib.ptr, self.adj
            args = (p(a.rowptr), p(a.col), self.n, self.nnz, p(self.dinv), 1.0, p(self.h[c]), c, p(self.b[c]), p(out), p(scratch), nbytes)

            def call():
                _lib.check(self.lib.pope_gcn_propagate(*args, sage._stream()))
                return out
            return call
        return self._raw(("propagate", c), build)

    def propagate_c256(self):
        return self._propagate(HIDDEN)

    def propagate_c7(self):
        return self._propagate(CLASSES)

    def conv_forward(self):
        def build():
            out = torch.empty((self.n, HIDDEN), dtype=torch.float32, device=self.dev)
            nbytes = self.lib.pope_gcn_conv_forward_scratch_size(self.n, self.nnz, C_IN, HIDDEN)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            p, a = _lib.ptr, self.adj
            args = (p(a.rowptr), p(a.col), self.n, self.nnz, p(self.dinv), 1.0, p(self.x), C_IN, p(self.weight), p(self.bias0), HIDDEN, p(out),
                    p(scratch), nbytes)

            def call():
                _lib.check(self.lib.pope_gcn_conv_forward(*args, sage._stream()))
                return out
            return call
        return self._raw("forward", build)

    def conv_backward(self):
        def build():
            gx = torch.empty_like(self.x)
            gw, gb = torch.empty_like(self.weight), torch.empty(HIDDEN, dtype=torch.float32, device=self.dev)
            nbytes = self.lib.pope_gcn_conv_backward_scratch_size(self.n, self.nnz, C_IN, HIDDEN)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            p, a = _lib.ptr, self.adj
            args = (p(a.rowptr_t), p(a.col_t), self.n, self.nnz, p(self.dinv), 1.0, p(self.x), C_IN, p(self.weight), HIDDEN, p(self.g_out), p(gx),
                    p(gw), p(gb), p(scratch), nbytes)

            def call():
                _lib.check(self.lib.pope_gcn_conv_backward(*args, sage._stream()))
                return gx, gw, gb
            return call
        return self._raw("backward", build)

    def train_step(self):
        for p in self.model.parameters():
            p.grad = None
        loss = sage.cross_entropy(self.model(self.x, self.adj).index_select(0, self.train_rows), self.y_train)
        loss.backward()
        self.opt.step()
        return loss

    def kernel_names(self, cus):
        names = {}
        for key, (c_in, c_out, backward) in {"conv_forward": (C_IN, HIDDEN, 0), "conv_backward": (C_IN, HIDDEN, 1), "layer1_forward": (HIDDEN, CLASSES, 0),
                                             "layer1_backward": (HIDDEN, CLASSES, 1)}.items():
            b = ctypes.create_string_buffer(512)
            _lib.check(self.lib.pope_gcn_kernel_name(self.n, self.nnz, c_in, c_out, backward, 1, cus, 0, b, 512))
            names[key] = b.value.decode()
        return names


FORMS = ("propagate_c256", "propagate_c7", "conv_forward", "conv_backward", "train_step")


def recorded_aggregate(name):
    """The aggregate launches of sage_full_layer_forward's layer 1 (width 256, no BatchNorm) from profiles/full_inference_times.json."""
    try:
        with open(os.path.join(ROOT, "profiles", "full_inference_times.json")) as f:
            launches = json.load(f)["graphs"][name]["launches"][1]
        return {k: v["average_us"] for k, v in launches.items() if k.startswith("k_full_") and k != "k_full_prepare"}
    except (OSError, KeyError, TypeError, IndexError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--graphs", default="flickr,pubmed")
    ap.add_argument("--time-limit", type=int, default=420, help="seconds after which the run ends itself")
    ap.add_argument("--trace", nargs=2, metavar=("GRAPH", "FORM"), default=None, help="only run one form --steps times (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.time_limit, exit=True)
    dev = engine.require_gpu()
    if args.trace:
        fn = getattr(World(args.trace[0], dev), args.trace[1])
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        print("traced", *args.trace, args.steps, "calls")
        return
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def stats(ts):
        return {"median": float(np.median(ts)), "min": min(ts), "max": max(ts), "all": ts}

    res = {"shape": {"in_channels": C_IN, "hidden": HIDDEN, "classes": CLASSES, "model": "GCN(756, 256, 7), 2 layers, dropout 0.5"},
           "calls_per_block": args.steps, "warmup_calls": args.warmup, "reps": args.reps, "unit": "us per call, HIP events around a block",
           "device": torch.cuda.get_device_name(0), "compute_units": cus, "graphs": {}}
    for name in args.graphs.split(","):
        w = World(name, dev)
        bwd, tbwd = w.conv_backward(), w.torch_conv_backward()
        agreement = {"propagate_c256": rel_err(w.propagate_c256(), w.torch_propagate_c256()), "propagate_c7": rel_err(w.propagate_c7(), w.torch_propagate_c7()),
                     "conv_forward": rel_err(w.conv_forward(), w.torch_conv_forward()),
                     "conv_backward": max(rel_err(a, b) for a, b in zip(bwd, tbwd))}
        assert max(agreement.values()) < 1e-4, agreement
        forms = {}
        for k in FORMS:
            forms[k], forms["torch_" + k] = getattr(w, k), getattr(w, "torch_" + k)
        for fn in forms.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, fn in forms.items():
                times[k].append(events_us(fn, args.steps))
        out = {"nodes": w.n, "slots": w.nnz, "max_relative_difference": agreement, "launch_lists": w.kernel_names(cus),
               "forms": {k: stats(ts) for k, ts in times.items()}, "beats_torch_with_disjoint_ranges": {}, "propagate_bandwidth": {}}
        for k in FORMS:
            out["beats_torch_with_disjoint_ranges"][k] = bool(out["forms"][k]["max"] < out["forms"]["torch_" + k]["min"])
        for c in (HIDDEN, CLASSES):
            nbytes = w.nnz * c * 4 + 2 * w.n * c * 4 + 8 * w.nnz
            us = out["forms"]["propagate_c%d" % c]["median"]
            out["propagate_bandwidth"]["c%d" % c] = {"model_bytes": nbytes, "achieved_bytes_per_s": nbytes / (us * 1e-6)}
        out["sage_full_aggregate_c256_recorded_us"] = recorded_aggregate(name) or "not recorded"
        res["graphs"][name] = out
        del w, forms, fn                                               # (the torch model and the world hold one another)
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
