#!/usr/bin/env python3
"""Time the SAGE training step in the default and in the deterministic mode (sage.set_deterministic), at bench.py's shape: 1550
seeds, fan-out [25, 10], 756 input columns, hidden 256, 3 layers, batches from a pre-sampled pool.  All in this one process:

    step           SageTrainStep over Adam(max_grad_norm=0.5), mode off and on, each enqueued eagerly and replayed as a HIP graph
    layer_backward sage_conv_backward of the hidden layer on the inner block of one batch (1550 destinations, 256 -> 256, with an input
                   gradient), mode off and on: the two differ in the grad_x chain alone (k_gemm_dual's zeroing + k_scatter_and_finals
                   against k_bwd_finals + index build + k_scatter_sum_det)
    sum_alone      sage_scatter_mean_det on the same block: the index build and the sum without anything else
    lists          the lengths of the per-source lists of that block (median and maximum over the listed sources, lists longer than a
                   wave): whether hub rows need chunking

A figure is the time between two HIP events around a block of calls, divided by the calls; --reps blocks per form, taken in turns
(form after form, then the next repetition) so that drift of the machine lands on all forms alike; min / median / max per form.
The run ends itself after --time-limit seconds; run it under `timeout` too.  Prints one JSON object; --out FILE also writes it
there (DESIGN: profiles/deterministic_step_times.json)."""
import argparse
import ctypes
import faulthandler
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphpope_amd import _lib, engine, sage, synth  # noqa: E402
from graphpope_amd.optim import Adam  # noqa: E402
from graphpope_amd.sage import SAGE, sample_batch  # noqa: E402
from graphpope_amd.sampler import DeviceBatch  # noqa: E402
from graphpope_amd.train import SageTrainStep  # noqa: E402

BATCH, SIZES, C_IN, HIDDEN, LAYERS, CLASSES = 1550, (25, 10), 756, 256, 3, 7


def make_pool(dev, n_batches=8):
    ei, n = synth.flickr_like(seed=1)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=n))])
    rng = np.random.default_rng(0)
    pool, inner = [], None
    for b in range(n_batches):
        seeds = rng.choice(n, BATCH, replace=False)
        n_id, adjs = sample_batch(rowptr, ei[1], seeds, sizes=SIZES, rng=rng)
        inner = inner or adjs[-1]
        db = DeviceBatch(BATCH, SIZES, dev)
        db.load(torch.as_tensor(n_id, device=dev), [a.to(dev) for a in adjs])
        pool.append((db, torch.randint(0, CLASSES, (BATCH,), device=dev, generator=torch.Generator(device=dev).manual_seed(b))))
    feats = torch.rand(n, C_IN, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    return feats, pool, inner


def timed_us(fn, k):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(k):
        fn()
    t1.record()
    t1.synchronize()
    return 1e3 * t0.elapsed_time(t1) / k


class Step:
    """The training step under one mode; the mode is set around every call, since it is read when launches are enqueued."""

    def __init__(self, on, use_graph, feats, pool, dev):
        self.on, self.pool, self.i = on, pool, 0
        torch.manual_seed(0)
        self.model = SAGE(C_IN, CLASSES, HIDDEN, LAYERS).to(dev)
        self.opt = Adam(self.model.parameters(), lr=1e-3, max_grad_norm=0.5)
        with sage.deterministic(on):
            self.trainer = SageTrainStep(self.model, self.opt, feats, BATCH, SIZES, sampler=None, clip=None, graph=use_graph)

    def one(self):
        db, y = self.pool[self.i % len(self.pool)]
        self.i += 1
        self.trainer.load_batch(db, y)
        self.trainer.run()

    def block_us(self, k):
        with sage.deterministic(self.on):
            return timed_us(self.one, k)


class LayerBackward:
    """sage_conv_backward of the hidden layer on one inner block, buffers owned here (scratch sized under the mode)."""

    def __init__(self, on, adj, dev):
        self.on, self.lib = on, _lib.load()
        adj = adj.to(dev)
        self.adj, n_dst, n_src, c = adj, adj.n_dst, adj.n_src, HIDDEN
        g = torch.Generator(device=dev).manual_seed(3)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)
        self.x, self.agg, self.w_l, self.w_r, self.grad_out = r(n_src, c), r(n_dst, c), r(c, c), r(c, c), r(n_dst, c)
        self.grad_x, self.grad_w_l, self.grad_w_r, self.grad_b = r(n_src, c), r(c, c), r(c, c), r(c)
        with sage.deterministic(on):
            self.nbytes = self.lib.sage_conv_scratch_bytes(n_src, n_dst, adj.col.numel(), c, c)
        self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)

    def one(self):
        p, a, c = _lib.ptr, self.adj, HIDDEN
        _lib.check(self.lib.sage_conv_backward(p(a.rowptr), p(a.col), a.n_src, a.n_dst, a.col.numel(), p(self.x), p(self.agg), c, p(self.w_l),
                                               p(self.w_r), c, p(self.grad_out), p(self.grad_x), p(self.grad_w_l), p(self.grad_b),
                                               p(self.grad_w_r), p(self.scratch), self.nbytes, None,
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def block_us(self, k):
        with sage.deterministic(self.on):
            return timed_us(self.one, k)


class SumAlone(LayerBackward):
    def __init__(self, adj, dev):
        super().__init__(True, adj, dev)
        self.nbytes = self.lib.sage_scatter_mean_det_scratch_bytes(self.adj.n_src, self.adj.n_dst, self.adj.col.numel())
        self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)

    def one(self):
        p, a = _lib.ptr, self.adj
        _lib.check(self.lib.sage_scatter_mean_det(p(a.rowptr), p(a.col), a.n_src, a.n_dst, a.col.numel(), p(self.agg), HIDDEN, p(self.grad_x),
                                                  p(self.scratch), self.nbytes, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=20, help="calls per form before the first timed block (>= 4: two eager calls, the capture, a replay)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=420, help="seconds after which the run ends itself")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.time_limit, exit=True)
    dev = engine.require_gpu()
    torch.autograd.set_multithreading_enabled(False)             # as graphpope_amd.main does: backward in the calling thread
    feats, pool, inner = make_pool(dev)
    forms = {}
    for mode in ("eager", "replayed"):
        for on in (False, True):
            forms["step_%s_%s" % (mode, "on" if on else "off")] = Step(on, mode == "replayed", feats, pool, dev)
    for on in (False, True):
        forms["layer_backward_%s" % ("on" if on else "off")] = LayerBackward(on, inner, dev)
    forms["sum_alone"] = SumAlone(inner, dev)
    for f in forms.values():
        f.block_us(max(args.warmup, 4))
    times = {key: [] for key in forms}
    for _ in range(args.reps):
        for key, f in forms.items():
            times[key].append(f.block_us(args.steps))
    assert not sage.is_deterministic()
    in_deg = np.bincount(inner.col.cpu().numpy(), minlength=inner.n_src)
    listed = in_deg[in_deg > 0]
    res = {"shape": {"seeds": BATCH, "fan_out": list(SIZES), "in_channels": C_IN, "hidden": HIDDEN, "layers": LAYERS, "batches": "pre-sampled pool of 8",
                     "inner_block": {"n_dst": inner.n_dst, "n_src": inner.n_src, "nnz": int(inner.col.numel())}},
           "calls_per_block": args.steps, "warmup_calls": max(args.warmup, 4), "reps": args.reps, "unit": "us per call, HIP events around a block",
           "forms": {key: {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "all": ts} for key, ts in times.items()},
           "lists": {"sources": int(inner.n_src), "listed_sources": int(listed.size), "median": float(np.median(listed)), "max": int(listed.max()),
                     "longer_than_64": int((in_deg > 64).sum()), "mean": float(listed.mean())}}
    med = lambda key: res["forms"][key]["median"]
    res["median_differences_us"] = {"step_eager_on_minus_off": med("step_eager_on") - med("step_eager_off"),
                                    "step_replayed_on_minus_off": med("step_replayed_on") - med("step_replayed_off"),
                                    "layer_backward_on_minus_off": med("layer_backward_on") - med("layer_backward_off")}
    for key in ("step_eager_off", "step_eager_on", "step_replayed_off", "step_replayed_on"):
        loss = float(forms[key].trainer.loss)
        assert np.isfinite(loss), key
        res["forms"][key]["last_loss"] = loss
    res["device"] = torch.cuda.get_device_name(0)
    faulthandler.cancel_dump_traceback_later()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
