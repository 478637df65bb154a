#!/usr/bin/env python3
"""Time an evaluation batch of graphpope_amd.main (main.py:224-241 validation_step / test_step) at the Flickr shape: synth.flickr_like(),
500 + 256 input columns, 1550 seeds, fan-out [25, 10], hidden 256, num_layers 3.  Everything in this one process on one GPU:

    (a) eager_batch      the batch as the eager evaluation loop runs it: sampler.sample (host-sized: it synchronises and reads the batch
                         sizes back), the model launch by launch, cross_entropy, then the torch metric chain
                         (loss * n, +=, argmax, ==, sum, +=)
    (b) replayed_batch   the same batch as one replay of train.SageEvalStep (device-extent sampler, forward pass, sage_eval_metrics and
                         the counter launch in one captured HIP graph)
    (c) metrics_kernel   sage_eval_metrics alone on [1550, 256] logits, against torch_chain: F.cross_entropy + the metric chain it
                         replaces
    (d) epoch            wall time of one training + validation epoch (main._run_epoch twice, read-backs included) with
                         GRAPHPOPE_EVAL_STEP=eager and with the default

(a)-(c): the time between two HIP events around a block of --steps calls, divided by the calls; (d): time.perf_counter around a
synchronised epoch.  --reps figures per form, the forms taken in turns (form after form, then the next repetition) so that drift of
the machine lands on all alike; min / median / max per form.  The run ends itself after --time-limit seconds; run it under
`timeout` too.  Prints one JSON object; --out FILE also writes it there (profiles/eval_step_times.json)."""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphpope_amd import engine, synth  # noqa: E402
from graphpope_amd import main as cli  # noqa: E402
from graphpope_amd.optim import Adam  # noqa: E402
from graphpope_amd.sage import SAGE, EvalMetrics, IndexedFeatures, cross_entropy  # noqa: E402
from graphpope_amd.sampler import NeighborSampler  # noqa: E402
from graphpope_amd.train import SageEvalStep, SageTrainStep  # noqa: E402

BATCH, SIZES, C_IN, HIDDEN, LAYERS, CLASSES = 1550, (25, 10), 756, 256, 3, 7


def events_us(fn, k):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(k):
        fn()
    t1.record()
    t1.synchronize()
    return 1e3 * t0.elapsed_time(t1) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="calls per timed block of (a)-(c)")
    ap.add_argument("--warmup", type=int, default=10, help="calls per form before the first timed block (>= 4: two eager calls, the capture, a replay)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--epoch-reps", type=int, default=3)
    ap.add_argument("--time-limit", type=int, default=420, help="seconds after which the run ends itself")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.time_limit, exit=True)
    dev = engine.require_gpu()
    torch.autograd.set_multithreading_enabled(False)             # as graphpope_amd.main does
    ei, n = synth.flickr_like()
    g = torch.Generator().manual_seed(0)
    feats = torch.rand(n, C_IN, generator=g).to(dev)
    labels = torch.randint(0, CLASSES, (n,), generator=g).to(dev)
    split = torch.rand(n, generator=g)
    idx = {"train": torch.nonzero(split < 0.5).flatten().to(dev), "val": torch.nonzero((split >= 0.5) & (split < 0.75)).flatten().to(dev)}
    adj_t = engine.build_csr(torch.as_tensor(ei).flip(0).contiguous().to(dev), n)
    sampler = NeighborSampler(adj_t.rowptr, adj_t.col, n, sizes=SIZES)
    torch.manual_seed(0)
    model = SAGE(C_IN, CLASSES, HIDDEN, LAYERS).to(dev)
    order = idx["val"]
    n_full = order.numel() // BATCH

    # (a) the eager evaluation batch, as main._run_epoch's eager path runs it
    state = {"b": 0, "tot_loss": torch.zeros((), device=dev), "tot_correct": torch.zeros((), device=dev, dtype=torch.int64)}

    def eager_batch():
        b = state["b"] % n_full
        state["b"] += 1
        seeds = order[b * BATCH:(b + 1) * BATCH]
        y = labels.index_select(0, seeds)
        n_id, adjs = sampler.sample(seeds, seed=(42 << 20) + b)
        with torch.no_grad():
            y_hat = model(IndexedFeatures(feats, n_id), adjs)
            loss = cross_entropy(y_hat, y)
        state["tot_loss"] += loss.detach() * seeds.numel()
        state["tot_correct"] += (y_hat.argmax(-1) == y).sum()

    # (b) the replayed batch
    ev = SageEvalStep(model, feats, BATCH, sampler)

    def replayed_batch():
        if not ev.batches_left():
            ev.begin_pass(order, labels, 42 << 20)                # once per n_full batches: one launch, inside the figure
        ev.step()

    # (c) the metrics alone, on the logits of a real batch
    model.eval()
    ev.begin_pass(order, labels, 42 << 20)
    logits, y_fix = ev.step().clone(), ev.y.clone()
    metrics = EvalMetrics(dev)

    def metrics_kernel():
        metrics.update(logits, y_fix)

    def torch_chain():
        loss = F.cross_entropy(logits, y_fix)
        state["tot_loss"] += loss * y_fix.numel()
        state["tot_correct"] += (logits.argmax(-1) == y_fix).sum()

    forms = {"eager_batch": eager_batch, "replayed_batch": replayed_batch, "metrics_kernel": metrics_kernel, "torch_chain": torch_chain}
    for fn in forms.values():
        for _ in range(max(args.warmup, 4)):
            fn()
    torch.cuda.synchronize()
    assert ev._graph is not None
    times = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, fn in forms.items():
            times[name].append(events_us(fn, args.steps))
    # the two paths saw the same batches: their figures agree
    ref_loss, ref_acc = cli._run_epoch(model, feats, labels, sampler, order, argparse.Namespace(batch_size=BATCH, seed=42), None, 0)
    got_loss, got_acc = ev.run_pass(order, labels, 42 << 20)
    assert abs(got_loss - ref_loss) <= 1e-5 * abs(ref_loss) and abs(got_acc - ref_acc) <= 0.01, (got_loss, ref_loss, got_acc, ref_acc)

    # (d) one training + validation epoch, both ways, on one model / optimiser / trainer
    opt = Adam(model.parameters(), lr=1e-3, max_grad_norm=0.5)
    trainer = SageTrainStep(model, opt, feats, BATCH, sampler=sampler, clip=None, seed=42)
    gen = torch.Generator(device=dev).manual_seed(42)
    ns = argparse.Namespace(batch_size=BATCH, seed=42)
    epoch_no = [0]

    def epoch(evaluator):
        e = epoch_no[0]
        epoch_no[0] += 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cli._run_epoch(model, feats, labels, sampler, idx["train"], ns, gen, e, opt, trainer)
        va = cli._run_epoch(model, feats, labels, sampler, order, ns, gen, e, evaluator=evaluator)
        torch.cuda.synchronize()
        assert np.isfinite(va[0])
        return 1e3 * (time.perf_counter() - t0)

    epoch_forms = {"eval_eager": None, "eval_replayed": ev}
    for evaluator in epoch_forms.values():
        epoch(evaluator)                                          # warm-up: the trainer's capture, the allocator
    epoch_ms = {name: [] for name in epoch_forms}
    for _ in range(args.epoch_reps):
        for name, evaluator in epoch_forms.items():
            epoch_ms[name].append(epoch(evaluator))

    def stats(ts):
        return {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "all": ts}

    res = {"shape": {"graph": "synth.flickr_like()", "nodes": n, "seeds": BATCH, "fan_out": list(SIZES), "in_channels": C_IN, "hidden": HIDDEN,
                     "layers": LAYERS, "val_nodes": int(order.numel()), "train_nodes": int(idx["train"].numel()),
                     "metrics_logits": list(logits.shape)},
           "calls_per_block": args.steps, "warmup_calls": max(args.warmup, 4), "reps": args.reps,
           "unit": "us per call, HIP events around a block", "forms": {name: stats(ts) for name, ts in times.items()},
           "epoch_unit": "ms per training + validation epoch, wall clock", "epoch_reps": args.epoch_reps,
           "epoch": {name: stats(ts) for name, ts in epoch_ms.items()},
           "val_pass_agreement": {"eager": [ref_loss, ref_acc], "replayed": [got_loss, got_acc]}}
    med = lambda name: res["forms"][name]["median"]  # noqa: E731
    res["median_ratios"] = {"eager_batch_over_replayed_batch": med("eager_batch") / med("replayed_batch"),
                            "torch_chain_over_metrics_kernel": med("torch_chain") / med("metrics_kernel"),
                            "epoch_eval_eager_over_eval_replayed": res["epoch"]["eval_eager"]["median"] / res["epoch"]["eval_replayed"]["median"]}
    res["device"] = torch.cuda.get_device_name(0)
    faulthandler.cancel_dump_traceback_later()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
