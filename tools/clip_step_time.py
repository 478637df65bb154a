#!/usr/bin/env python3
"""Time the SAGE training step with and without gradient-norm clipping (main.py:285-290 gradient_clip_val=0.5), at bench.py's
shape: 1550 seeds, fan-out [25, 10], 756 input columns, hidden 256, 3 layers, batches from a pre-sampled pool.  Three forms, each
both enqueued eagerly (graph=False) and replayed as a HIP graph, all in this one process:

    no_clip      SageTrainStep(clip=None) over Adam()                       -- what bench.py times
    torch_clip   SageTrainStep(clip=0.5) over Adam()                        -- torch.nn.utils.clip_grad_norm_ in front of the step
    fused_clip   SageTrainStep(clip=None) over Adam(max_grad_norm=0.5)      -- sage_grad_sqnorm + sage_adam_step_clip

A figure is the time between two HIP events around a block of --steps steps, divided by the steps; --reps blocks per form, taken
in turns (form after form, then the next repetition) so that drift of the machine lands on all forms alike.  min / median / max
per form, and the differences of the medians.  The whole run ends itself after --time-limit seconds; run it under `timeout` too.
Prints one JSON object; --out FILE also writes it there (DESIGN: profiles/clip_step_times.json)."""
import argparse
import faulthandler
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphpope_amd import engine, synth  # noqa: E402
from graphpope_amd.optim import Adam  # noqa: E402
from graphpope_amd.sage import SAGE, sample_batch  # noqa: E402
from graphpope_amd.sampler import DeviceBatch  # noqa: E402
from graphpope_amd.train import SageTrainStep  # noqa: E402

BATCH, SIZES, C_IN, HIDDEN, LAYERS, CLASSES = 1550, (25, 10), 756, 256, 3, 7
FORMS = {"no_clip": (None, None), "torch_clip": (0.5, None), "fused_clip": (None, 0.5)}      # (SageTrainStep clip, Adam max_grad_norm)


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


class Form:
    def __init__(self, name, use_graph, feats, pool, dev):
        clip, max_grad_norm = FORMS[name]
        torch.manual_seed(0)
        self.model = SAGE(C_IN, CLASSES, HIDDEN, LAYERS).to(dev)
        self.opt = Adam(self.model.parameters(), lr=1e-3, max_grad_norm=max_grad_norm)
        self.trainer = SageTrainStep(self.model, self.opt, feats, BATCH, SIZES, sampler=None, clip=clip, graph=use_graph)
        self.pool, self.i = pool, 0

    def steps(self, k):
        for _ in range(k):
            db, y = self.pool[self.i % len(self.pool)]
            self.i += 1
            self.trainer.load_batch(db, y)
            self.trainer.run()

    def block_us(self, k):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        self.steps(k)
        t1.record()
        t1.synchronize()
        return 1e3 * t0.elapsed_time(t1) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=20, help="steps per form before the first timed block (>= 4: two eager calls, the capture, a replay)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=420, help="seconds after which the run ends itself")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.time_limit, exit=True)
    dev = engine.require_gpu()
    torch.autograd.set_multithreading_enabled(False)             # as graphpope_amd.main does: backward in the calling thread
    feats, pool = make_pool(dev)
    forms = {(name, mode): Form(name, mode == "replayed", feats, pool, dev) for name in FORMS for mode in ("eager", "replayed")}
    for f in forms.values():
        f.steps(max(args.warmup, 4))
    torch.cuda.synchronize()
    times = {key: [] for key in forms}
    for _ in range(args.reps):
        for key, f in forms.items():
            times[key].append(f.block_us(args.steps))
    res = {"shape": {"seeds": BATCH, "fan_out": list(SIZES), "in_channels": C_IN, "hidden": HIDDEN, "layers": LAYERS,
                     "parameters": sum(p.numel() for p in forms[("no_clip", "eager")].model.parameters()),
                     "parameter_tensors": len(list(forms[("no_clip", "eager")].model.parameters())), "batches": "pre-sampled pool of 8"},
           "steps_per_block": args.steps, "warmup_steps": max(args.warmup, 4), "reps": args.reps, "unit": "us per step, HIP events around a block",
           "forms": {name: {} for name in FORMS}}
    for (name, mode), ts in times.items():
        loss = float(forms[(name, mode)].trainer.loss)
        assert np.isfinite(loss), (name, mode)
        res["forms"][name][mode] = {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "all": ts, "last_loss": loss}
    med = lambda name, mode: res["forms"][name][mode]["median"]
    res["median_differences_us"] = {mode: {"torch_clip_minus_no_clip": med("torch_clip", mode) - med("no_clip", mode),
                                           "fused_clip_minus_no_clip": med("fused_clip", mode) - med("no_clip", mode),
                                           "fused_clip_minus_torch_clip": med("fused_clip", mode) - med("torch_clip", mode)}
                                    for mode in ("eager", "replayed")}
    opt = forms[("fused_clip", "replayed")].opt
    res["fused_clip_last_norm_and_coefficient"] = [float(opt.grad_norm), float(opt.clip_coef)]
    res["device"] = torch.cuda.get_device_name(0)
    faulthandler.cancel_dump_traceback_later()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
