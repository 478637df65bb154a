#!/usr/bin/env python3
"""Time what data-parallel training adds to the eager SAGE training step (graphpope_amd.parallel.GradBucket), at bench.py's shape: 1550
seeds, fan-out [25, 10], 756 input columns, hidden 256, 3 layers, batches from a pre-sampled pool, the clip inside the optimiser.

    plain     SageTrainStep(graph=False) over Adam(max_grad_norm=0.5)                          -- the parent's eager step
    bucket    the same step with GradBucket.sync(force=True) between backward() and opt.step(), on a world-1 nccl group: the pack launch,
              one RCCL all-reduce of the bucket, the gradients installed as views
    pack      the pack launch alone, over the gradients of the last step

plain and bucket run in this one process and take turns (a block of one, a block of the other, then the next repetition), so drift of
the machine lands on both alike; median [min - max] of --reps blocks.  A figure is the time between two HIP events around a block of
--steps steps, divided by the steps.  For information only, a third figure: two ranks on this one card over gloo (which stages the
bucket through the host), each on its own batches -- rank 0's wall time per step.  It runs first, in child processes of their own, before
this process touches the GPU.  No threshold is set on any of these; the expectation to read them against is `plain` of the same run.
Nothing here runs on more than one GPU.  The whole run ends itself after --time-limit seconds; run it under `timeout` too.
Prints one JSON object; --out FILE also writes it there (profiles/ddp_step_times.json)."""
import argparse
import faulthandler
import json
import os
import socket
import sys
import tempfile
import time

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

BATCH, SIZES, C_IN, HIDDEN, LAYERS, CLASSES = 1550, (25, 10), 756, 256, 3, 7


def make_step(dev, feats, group=None):
    from graphpope_amd.optim import Adam
    from graphpope_amd.sage import SAGE
    from graphpope_amd.train import SageTrainStep
    torch.manual_seed(0)
    model = SAGE(C_IN, CLASSES, HIDDEN, LAYERS).to(dev)
    opt = Adam(model.parameters(), lr=1e-3, max_grad_norm=0.5)
    return model, opt, SageTrainStep(model, opt, feats, BATCH, SIZES, sampler=None, graph=False, group=group)


class Form:
    def __init__(self, dev, feats, pool, group=None, force=False, first=0, stride=1):
        from graphpope_amd.parallel import GradBucket
        self.model, self.opt, self.trainer = make_step(dev, feats, group)
        if force:                                                    # world 1: the step's own hook, with the collective forced
            bucket = GradBucket(self.trainer.params)
            sync = bucket.sync
            bucket.sync = lambda g=None: sync(g, force=True)
            self.trainer.group, self.trainer.bucket = group, bucket
        self.pool, self.i, self.stride = pool, first, stride

    def steps(self, k):
        for _ in range(k):
            db, y = self.pool[self.i % len(self.pool)]
            self.i += self.stride
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


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def summary(ts):
    return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "all": ts}


def _gloo_rank(rank, world, port, steps, warmup, reps, out_path):
    from clip_step_time import make_pool
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda", 0)
        torch.autograd.set_multithreading_enabled(False)
        feats, pool = make_pool(dev)
        form = Form(dev, feats, pool, group=dist.group.WORLD, first=rank, stride=world)
        form.steps(warmup)
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            dist.barrier()
            t = time.perf_counter()
            form.steps(steps)
            torch.cuda.synchronize()
            ts.append(1e6 * (time.perf_counter() - t) / steps)
        if rank == 0:
            with open(out_path, "w") as f:
                json.dump(dict(summary(ts), last_loss=float(form.trainer.loss)), f)
    finally:
        dist.destroy_process_group()


def gloo_two_ranks(steps, warmup, reps, limit):
    port = free_port()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "rank0.json")
        ctx = mp.spawn(_gloo_rank, args=(2, port, steps, warmup, reps, out), nprocs=2, join=False)
        end, done = time.monotonic() + limit, False
        try:
            while not done and time.monotonic() < end:
                done = ctx.join(timeout=1.0)
        finally:
            if not done:
                for p in ctx.processes:
                    if p.is_alive():
                        p.terminate()
        if not done:
            return {"error": f"the two ranks did not finish within {limit} s"}
        return json.load(open(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=420, help="seconds after which the run ends itself")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.time_limit, exit=True)
    gloo = gloo_two_ranks(max(args.steps // 3, 10), args.warmup, args.reps, limit=args.time_limit // 2)

    from clip_step_time import make_pool
    from graphpope_amd import engine
    dev = engine.require_gpu()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        torch.autograd.set_multithreading_enabled(False)         # as graphpope_amd.main does: backward in the calling thread
        feats, pool = make_pool(dev)
        forms = {"plain": Form(dev, feats, pool), "bucket": Form(dev, feats, pool, group=dist.group.WORLD, force=True)}
        for f in forms.values():
            f.steps(args.warmup)
        torch.cuda.synchronize()
        times = {key: [] for key in forms}
        for _ in range(args.reps):
            for key, f in forms.items():
                times[key].append(f.block_us(args.steps))
        bucket = forms["bucket"].trainer.bucket
        for p in bucket.live:                                       # the pack alone, from gradients outside the bucket as backward() leaves them
            p.grad = p.grad.clone()
        pack = []
        for _ in range(args.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(args.steps):
                bucket.pack(1.0)
            t1.record()
            t1.synchronize()
            pack.append(1e3 * t0.elapsed_time(t1) / args.steps)
        res = {"shape": {"seeds": BATCH, "fan_out": list(SIZES), "in_channels": C_IN, "hidden": HIDDEN, "layers": LAYERS,
                         "bucket_elements": int(bucket.flat.numel()), "bucket_tensors": len(bucket.live), "batches": "pre-sampled pool of 8"},
               "steps_per_block": args.steps, "warmup_steps": args.warmup, "reps": args.reps,
               "unit": "us per step; HIP events around a block (plain, bucket, pack), wall clock of rank 0 (gloo_two_ranks_one_card)",
               "plain": dict(summary(times["plain"]), last_loss=float(forms["plain"].trainer.loss)),
               "bucket": dict(summary(times["bucket"]), last_loss=float(forms["bucket"].trainer.loss)),
               "bucket_minus_plain_median_us": float(np.median(times["bucket"]) - np.median(times["plain"])),
               "pack": summary(pack),
               "gloo_two_ranks_one_card": dict(gloo, steps_per_block=max(args.steps // 3, 10), note="for information only"),
               "not_measured": "more than one GPU; RCCL with more than one rank; any scaling",
               "device": torch.cuda.get_device_name(0)}
    finally:
        dist.destroy_process_group()
    faulthandler.cancel_dump_traceback_later()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
