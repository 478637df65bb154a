#!/usr/bin/env python3
"""Time the row L2 normalisation (sage_l2_normalize_forward / _backward, csrc/l2norm.hip) and what it costs a training step.  All in
this one process:

    kernel_forward / kernel_backward   the two launches alone at [40 300, 256] (the outer block of bench.py's SAGE shape: 1 550 seeds
                                       times 1 + 25 neighbours) and at [1 550, 256] (the inner block), out of place
    torch_forward / torch_backward     torch.nn.functional.normalize(x, p=2, dim=-1, eps=1e-12) and its autograd backward pass on the
                                       same tensors
    step_replayed_off / _on            the replayed SageTrainStep of bench.py's SAGE shape (1550 seeds, fan-out [25, 10], 756 input
                                       columns, hidden 256, 3 layers, Adam with the clip inside, batches from a pre-sampled pool) with
                                       normalize=False and with normalize=True

A figure is the time between two HIP events around a block of calls, divided by the calls; --reps blocks per form, taken in turns (form
after form, then the next repetition) so that drift of the machine lands on all forms alike; min / median / max per form.  The bytes a
kernel must move are computed from the shape (forward: read 4 M C, write 4 M C + 4 M; backward: read 8 M C + 4 M, write 4 M C) and set
against the float4 copy rate measured on this chip, 6.29 TB/s.  The run ends itself after --time-limit seconds; run it under `timeout`
too.  Prints one JSON object; --out FILE also writes it there (profiles/l2norm_times.json)."""
import argparse
import ctypes
import faulthandler
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphpope_amd import _lib, engine, synth  # noqa: E402
from graphpope_amd.optim import Adam  # noqa: E402
from graphpope_amd.sage import L2_EPS, SAGE, sample_batch  # noqa: E402
from graphpope_amd.sampler import DeviceBatch  # noqa: E402
from graphpope_amd.train import SageTrainStep  # noqa: E402

BATCH, SIZES, C_IN, HIDDEN, LAYERS, CLASSES = 1550, (25, 10), 756, 256, 3, 7
SHAPES = ((40300, 256), (1550, 256))
COPY_RATE = 6.29e12                     # bytes / s, float4 copy


def make_pool(dev, n_batches=8):
    ei, n = synth.flickr_like(seed=1)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=n))])
    rng = np.random.default_rng(0)
    pool = []
    for b in range(n_batches):
        seeds = rng.choice(n, BATCH, replace=False)
        n_id, adjs = sample_batch(rowptr, ei[1], seeds, sizes=SIZES, rng=rng)
        db = DeviceBatch(BATCH, SIZES, dev)
        db.load(torch.as_tensor(n_id, device=dev), [a.to(dev) for a in adjs])
        pool.append((db, torch.randint(0, CLASSES, (BATCH,), device=dev, generator=torch.Generator(device=dev).manual_seed(b))))
    feats = torch.rand(n, C_IN, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    return feats, pool


def timed_us(fn, k):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(k):
        fn()
    t1.record()
    t1.synchronize()
    return 1e3 * t0.elapsed_time(t1) / k


class Kernels:
    """The two entry points and torch's ops on one set of tensors of a shape."""

    def __init__(self, m, c, dev):
        self.lib, self.m, self.c = _lib.load(), m, c
        g = torch.Generator(device=dev).manual_seed(m)
        self.x = torch.randn(m, c, device=dev, generator=g)
        self.g = torch.randn(m, c, device=dev, generator=g)
        self.y, self.gx = torch.empty_like(self.x), torch.empty_like(self.x)
        self.inv = torch.empty(m, device=dev)
        self.xt = self.x.clone().requires_grad_(True)
        self.forward()
        self.yt = F.normalize(self.xt, p=2.0, dim=-1, eps=L2_EPS)

    def forward(self):
        p = _lib.ptr
        _lib.check(self.lib.sage_l2_normalize_forward(p(self.x), self.m, self.c, L2_EPS, p(self.y), p(self.inv), None,
                                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def backward(self):
        p = _lib.ptr
        _lib.check(self.lib.sage_l2_normalize_backward(p(self.y), p(self.inv), p(self.g), self.m, self.c, L2_EPS, p(self.gx), None,
                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def torch_forward(self):
        with torch.no_grad():
            F.normalize(self.x, p=2.0, dim=-1, eps=L2_EPS)

    def torch_backward(self):
        torch.autograd.grad(self.yt, self.xt, self.g, retain_graph=True)

    def agreement(self):
        """max |ours - torch| of the output and of the gradient: the forms that are timed compute the same thing."""
        gt, = torch.autograd.grad(self.yt, self.xt, self.g, retain_graph=True)
        self.backward()
        return float((self.y - self.yt.detach()).abs().max()), float((self.gx - gt).abs().max() / gt.abs().max())


class Form:
    def __init__(self, fn):
        self.fn = fn

    def block_us(self, k):
        return timed_us(self.fn, k)


class Step(Form):
    def __init__(self, normalize, feats, pool, dev):
        self.pool, self.i = pool, 0
        torch.manual_seed(0)
        self.model = SAGE(C_IN, CLASSES, HIDDEN, LAYERS, normalize=normalize).to(dev)
        self.opt = Adam(self.model.parameters(), lr=1e-3, max_grad_norm=0.5)
        self.trainer = SageTrainStep(self.model, self.opt, feats, BATCH, SIZES, sampler=None, clip=None, graph=True)
        self.fn = self.one

    def one(self):
        db, y = self.pool[self.i % len(self.pool)]
        self.i += 1
        self.trainer.load_batch(db, y)
        self.trainer.run()


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
    forms, kernels = {}, {}
    for m, c in SHAPES:
        k = kernels[m, c] = Kernels(m, c, dev)
        tag = "%dx%d" % (m, c)
        forms["kernel_forward_" + tag], forms["kernel_backward_" + tag] = Form(k.forward), Form(k.backward)
        forms["torch_forward_" + tag], forms["torch_backward_" + tag] = Form(k.torch_forward), Form(k.torch_backward)
    feats, pool = make_pool(dev)
    forms["step_replayed_off"], forms["step_replayed_on"] = Step(False, feats, pool, dev), Step(True, feats, pool, dev)
    for f in forms.values():
        f.block_us(max(args.warmup, 4))
    times = {key: [] for key in forms}
    for _ in range(args.reps):
        for key, f in forms.items():
            times[key].append(f.block_us(args.steps))
    res = {"shape": {"seeds": BATCH, "fan_out": list(SIZES), "in_channels": C_IN, "hidden": HIDDEN, "layers": LAYERS, "batches": "pre-sampled pool of 8"},
           "calls_per_block": args.steps, "warmup_calls": max(args.warmup, 4), "reps": args.reps, "unit": "us per call, HIP events around a block",
           "forms": {key: {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "all": ts} for key, ts in times.items()},
           "copy_rate_bytes_per_s": COPY_RATE, "kernels": {}}
    med = lambda key: res["forms"][key]["median"]
    for (m, c), k in kernels.items():
        tag = "%dx%d" % (m, c)
        nbytes = {"forward": 8 * m * c + 4 * m, "backward": 12 * m * c + 4 * m}
        dy, dg = k.agreement()
        res["kernels"][tag] = {"max_abs_diff_y_vs_torch": dy, "rel_diff_grad_vs_torch": dg}
        for way in ("forward", "backward"):
            us = med("kernel_%s_%s" % (way, tag))
            res["kernels"][tag][way] = {"bytes": nbytes[way], "us_at_copy_rate": 1e6 * nbytes[way] / COPY_RATE,
                                        "fraction_of_copy_rate": nbytes[way] / (us * 1e-6) / COPY_RATE,
                                        "torch_over_kernel": med("torch_%s_%s" % (way, tag)) / us}
    res["step"] = {"on_minus_off_us": med("step_replayed_on") - med("step_replayed_off"), "on_over_off": med("step_replayed_on") / med("step_replayed_off")}
    for key in ("step_replayed_off", "step_replayed_on"):
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
