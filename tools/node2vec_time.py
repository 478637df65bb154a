#!/usr/bin/env python3
"""Time the node2vec training step (graphpope_amd.node2vec.Node2Vec.step) on the PubMed-shaped and the Flickr-shaped graph with the
hyper-parameters of /root/reference/generate_node2vec_embedding.py:23-25 (D 128, walk_length 20, context_size 10, walks_per_node 10,
one negative row per walk) and batches of 128 nodes.  Per graph, in one child process under a time limit:

    fused        ms per Node2Vec.step: HIP events around blocks of --steps steps, --reps blocks, taken in turns with `torch`
    torch        the same step out of stock torch ops on the same GPU: the walks as index_select chains over the CSR with torch.rand,
                 torch.randint negatives, PyG's window matrices and loss over torch.nn.Embedding(sparse=True) with autograd, and
                 torch.optim.SparseAdam
    epoch        ms of one pass over every node (Node2Vec.fit(1): host clock around work that ends in a synchronise)
    kernels      the step's split: HIP events between its launches (walks / loss_grad on the positive rows / on the negative rows /
                 sparse_adam), summed over a block of steps; each figure includes the gap in front of its launch
    atomic floor the bytes the two loss_grad launches add with float atomics (rows x (walk_length + 1) x D x 4) over the chip's measured
                 1.3 TB/s of added bytes, and the share of that floor the two launches reach
    deterministic  the step in the library's deterministic mode (sage.deterministic(): pope_n2v_position_grads + pope_n2v_accumulate_det
                 in place of pope_n2v_loss_grad) beside the step with the mode off, blocks taken in turns; the mode-on step's split by
                 call; and the hub case: pope_n2v_accumulate_det on the 53 760 entries of a step's rows with half of them on one node,
                 beside the same number of entries spread uniformly

--leg biased times the second-order walks instead (biased_run below: the walk launch alone, first-order beside (p, q) = (1, 1),
(0.25, 4), (4, 0.25); the share of steps that reached the exact pass; the training step on (0.25, 4) walks beside the first-order step).

The first child that fails ends the run.  Prints one JSON object; --out FILE also writes it there (DESIGN §7l:
profiles/node2vec_times.json; --leg biased: profiles/node2vec_biased_times.json)."""
import argparse
import faulthandler
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphpope_amd import synth  # noqa: E402

HP = dict(embedding_dim=128, walk_length=20, context_size=10, walks_per_node=10, num_negative_samples=1)
BATCH, LR = 128, 0.01
ATOMIC_BYTES_PER_SECOND = 1.3e12


def graph(name):
    if name == "flickr":
        return synth.flickr_like()
    if name == "pubmed":
        return synth.pubmed_like()
    raise SystemExit(f"unknown graph {name!r}")


class TorchStep:
    """The step written with stock torch ops only."""

    def __init__(self, model, dev):
        import torch
        self.torch, self.dev, self.n = torch, dev, model.num_nodes
        self.rowptr, self.col = model.csr.rowptr.long(), model.csr.col.long()
        self.emb = torch.nn.Embedding(self.n, HP["embedding_dim"], sparse=True).to(dev)
        self.opt = torch.optim.SparseAdam(self.emb.parameters(), lr=LR)
        self.gen = torch.Generator(device=dev).manual_seed(0)

    def windows(self, rows):
        c = HP["context_size"]
        return self.torch.cat([rows[:, j:j + c] for j in range(rows.shape[1] + 1 - c)], 0)

    def part(self, rw, negative):
        torch = self.torch
        start, rest = rw[:, 0], rw[:, 1:].contiguous()
        h_start = self.emb(start).view(rw.size(0), 1, -1)
        h_rest = self.emb(rest.view(-1)).view(rw.size(0), -1, h_start.shape[-1])
        out = (h_start * h_rest).sum(dim=-1).view(-1)
        return -torch.log((1 - torch.sigmoid(out) if negative else torch.sigmoid(out)) + 1e-15).mean()

    def step(self, batch):
        torch = self.torch
        starts = batch.repeat(HP["walks_per_node"])
        cur, cols = starts, [starts]
        for _ in range(HP["walk_length"]):
            lo = self.rowptr.index_select(0, cur)
            deg = self.rowptr.index_select(0, cur + 1) - lo
            pick = (torch.rand(cur.numel(), device=self.dev, generator=self.gen) * deg).long()
            pick = torch.minimum(pick, deg - 1).clamp_(min=0)                    # rand * deg can round up to deg; deg == 0 reads slot 0
            nxt = self.col.index_select(0, (lo + pick).clamp_(max=self.col.numel() - 1))
            cur = torch.where(deg > 0, nxt, cur)
            cols.append(cur)
        pos = torch.stack(cols, 1)
        neg = torch.cat([starts[:, None], torch.randint(self.n, (starts.numel(), HP["walk_length"]), device=self.dev, generator=self.gen)], 1)
        self.opt.zero_grad()
        loss = self.part(self.windows(pos), False) + self.part(self.windows(neg), True)
        loss.backward()
        self.opt.step()
        return loss.detach()


def deterministic_run(model, batches, steps, warmup, reps, off_block_ms):
    """The step in the library's deterministic mode beside the step with the mode off (blocks taken in turns, as above), the mode-on
    step's split by call, and the hub case: pope_n2v_accumulate_det on the entries of one step with half of them on one node."""
    import torch
    from graphpope_amd import node2vec, sage
    dev, count = model.device, [0]
    stat = lambda ts: {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "all": ts}

    def on_block_ms(k):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with sage.deterministic():
            t0.record()
            for _ in range(k):
                count[0] += 1
                loss = model.step(batches[count[0] % len(batches)], 50_000 + count[0])
            t1.record()
        t1.synchronize()
        assert bool(torch.isfinite(loss))
        return t0.elapsed_time(t1) / k

    on_block_ms(warmup)
    times = {"off": [], "on": []}
    for _ in range(reps):
        times["off"].append(off_block_ms(steps))
        times["on"].append(on_block_ms(steps))

    c, w, work = model.context_size, model.embedding.weight.data, model._det
    names = ("walks", "position_grads_pos", "accumulate_det_pos", "position_grads_neg", "accumulate_det_neg", "sparse_adam")
    marks = []
    torch.cuda.synchronize()
    for i in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        acc = model._loss_acc.zero_()
        ev[0].record()
        pos, neg = model.walks(batches[i % len(batches)], 20_000 + i)
        ev[1].record()
        at = 1
        for rows, negative in ((pos, False), (neg, True)):
            scale = 1.0 / node2vec._terms(rows, c)
            ids, contrib, row_loss = node2vec.position_grads(w, rows, c, negative, scale, work)
            ev[at + 1].record()
            node2vec.accumulate_det(ids, contrib, model.grad, model.touched, row_loss, scale, acc, work.scratch)
            ev[at + 2].record()
            at += 2
        model.step_count += 1
        node2vec.sparse_adam(w, model.grad, model.touched, model.exp_avg, model.exp_avg_sq, LR, 0.9, 0.999, 1e-8, model.step_count)
        ev[6].record()
        marks.append(ev)
    torch.cuda.synchronize()
    split = {nm: float(np.median([ev[k].elapsed_time(ev[k + 1]) for ev in marks])) for k, nm in enumerate(names)}

    # the hub case: the entries of one call at this shape (rows x len), every second one on node 0, the others spread
    n, d = w.shape
    m = 2 * BATCH * HP["walks_per_node"] * (HP["walk_length"] + 1)
    gen = torch.Generator().manual_seed(0)
    ids = torch.randint(1, n, (m,), generator=gen, dtype=torch.int32)
    ids[::2] = 0
    ids = ids.to(dev)
    contrib = torch.randn(m, d, generator=gen).to(dev)
    grad, touched = torch.zeros(n, d, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    scratch = torch.empty(_scratch_bytes(m, n), dtype=torch.uint8, device=dev)
    spread_ids = torch.randint(0, n, (m,), generator=gen, dtype=torch.int32).to(dev)
    hub, spread = [], []
    for which, out in ((ids, hub), (spread_ids, spread)):
        node2vec.accumulate_det(which, contrib, grad, touched, None, 1.0, None, scratch)       # warm-up
        for _ in range(reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            node2vec.accumulate_det(which, contrib, grad, touched, None, 1.0, None, scratch)
            t1.record()
            t1.synchronize()
            out.append(t0.elapsed_time(t1))
    return {"step_ms_mode_off": stat(times["off"]), "step_ms_mode_on": stat(times["on"]),
            "on_over_off": float(np.median(times["on"]) / np.median(times["off"])), "mode_on_split_ms_median": split,
            "hub_case": {"M": m, "entries_on_the_hub": int((ids == 0).sum()), "N": n, "D": d, "accumulate_det_ms": stat(hub),
                         "same_M_spread_uniformly_ms": stat(spread)}}


def _scratch_bytes(m, n):
    from graphpope_amd import _lib
    return _lib.load().pope_n2v_accumulate_det_scratch_bytes(m, n)


def gpu_run(name, steps, warmup, reps, time_limit):
    import torch
    from graphpope_amd import engine, node2vec
    faulthandler.dump_traceback_later(time_limit, exit=True)
    dev = engine.require_gpu()
    ei, n = graph(name)
    torch.manual_seed(0)
    model = node2vec.Node2Vec(torch.as_tensor(ei, device=dev), num_nodes=n, **HP)
    model.lr = LR
    stock = TorchStep(model, dev)
    order = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(dev)
    batches = [order[lo:lo + BATCH] for lo in range(0, n - BATCH + 1, BATCH)]
    count = {"fused": 0, "torch": 0}

    def run(form, k):
        loss = None
        for _ in range(k):
            b = batches[count[form] % len(batches)]
            count[form] += 1
            loss = model.step(b, count[form]) if form == "fused" else stock.step(b)
        return loss

    def block_ms(form, k):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        loss = run(form, k)
        t1.record()
        t1.synchronize()
        assert bool(torch.isfinite(loss)), form
        return t0.elapsed_time(t1) / k, float(loss)

    for form in count:
        run(form, warmup)
    times, last = {f: [] for f in count}, {}
    for _ in range(reps):
        for form in count:
            ms, last[form] = block_ms(form, steps)
            times[form].append(ms)
    det = deterministic_run(model, batches, steps, warmup, reps, lambda k: block_ms("fused", k)[0])

    # the step's split: events between the launches of `steps` steps
    c = model.context_size
    names = ("walks", "loss_grad_pos", "loss_grad_neg", "sparse_adam")
    marks = []
    w = model.embedding.weight.data
    torch.cuda.synchronize()
    for i in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        acc = model._loss_acc.zero_()
        ev[0].record()
        pos, neg = model.walks(batches[i % len(batches)], 10_000 + i)
        ev[1].record()
        node2vec.loss_grad(w, pos, c, False, 1.0 / node2vec._terms(pos, c), acc, model.grad, model.touched)
        ev[2].record()
        node2vec.loss_grad(w, neg, c, True, 1.0 / node2vec._terms(neg, c), acc, model.grad, model.touched)
        ev[3].record()
        model.step_count += 1
        node2vec.sparse_adam(w, model.grad, model.touched, model.exp_avg, model.exp_avg_sq, LR, 0.9, 0.999, 1e-8, model.step_count)
        ev[4].record()
        marks.append(ev)
    torch.cuda.synchronize()
    split = {nm: float(np.median([ev[k].elapsed_time(ev[k + 1]) for ev in marks])) for k, nm in enumerate(names)}
    rows = 2 * BATCH * HP["walks_per_node"]
    added = rows * (HP["walk_length"] + 1) * HP["embedding_dim"] * 4
    floor_ms = 1e3 * added / ATOMIC_BYTES_PER_SECOND
    loss_grad_ms = split["loss_grad_pos"] + split["loss_grad_neg"]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    epoch_loss = model.fit(1, batch_size=BATCH, lr=LR, seed=1)[0]
    torch.cuda.synchronize()
    epoch_ms = 1e3 * (time.perf_counter() - t0)
    faulthandler.cancel_dump_traceback_later()
    stat = lambda ts: {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "all": ts}
    return {"N": n, "E": int(ei.shape[1]), "hyper_parameters": HP, "batch": BATCH, "walk_rows_per_step": rows,
            "steps_per_block": steps, "warmup_steps": warmup, "reps": reps,
            "fused_ms_per_step": stat(times["fused"]), "torch_ms_per_step": stat(times["torch"]),
            "torch_over_fused": float(np.median(times["torch"]) / np.median(times["fused"])),
            "last_loss": last, "epoch_ms": epoch_ms, "epoch_steps": -(-n // BATCH), "epoch_mean_loss": epoch_loss,
            "kernel_split_ms_median": split, "atomic_bytes_added_per_step": added, "atomic_floor_ms": floor_ms,
            "loss_grad_ms": loss_grad_ms, "share_of_atomic_floor_reached": floor_ms / loss_grad_ms,
            "deterministic": det, "device": torch.cuda.get_device_name(0)}


BIASED_PQ = [(1.0, 1.0), (0.25, 4.0), (4.0, 0.25)]
BIASED_STEP_PQ = (0.25, 4.0)


def biased_run(name, steps, warmup, reps, time_limit):
    """--leg biased.  The walk launch alone at the reference's shape (BATCH x walks_per_node = 1 280 rows, 20 steps): pope_n2v_walks'
    positive rows beside pope_n2v_walks_biased for BIASED_PQ, all on the canonical CSR, blocks of --steps launches taken in turns; the
    share of steps that reached the exact pass, counted by the NumPy restatement of tests/node2vec_biased_cases.py on one batch (whose
    rows the launch has to equal); and the full training step of SecondOrderNode2Vec(BIASED_STEP_PQ) beside Node2Vec's."""
    import torch
    from graphpope_amd import engine, node2vec
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import node2vec_biased_cases as restatement
    faulthandler.dump_traceback_later(time_limit, exit=True)
    dev = engine.require_gpu()
    ei, n = graph(name)
    stat = lambda ts: {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "all": ts}
    torch.manual_seed(0)
    first = node2vec.Node2Vec(torch.as_tensor(ei, device=dev), num_nodes=n, **HP)
    torch.manual_seed(0)
    second = node2vec.SecondOrderNode2Vec(torch.as_tensor(ei, device=dev), num_nodes=n, p=BIASED_STEP_PQ[0], q=BIASED_STEP_PQ[1], **HP)
    first.lr = second.lr = LR
    csr, length = second.csr, HP["walk_length"]
    order = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(dev)
    batches = [order[lo:lo + BATCH].repeat(HP["walks_per_node"]) for lo in range(0, n - BATCH + 1, BATCH)]
    count = [0]

    def launch(form):
        count[0] += 1
        starts = batches[count[0] % len(batches)]
        if form == "first_order":
            return node2vec.walks(csr.rowptr, csr.col, n, starts, length, count[0], negative=False)[0]
        return node2vec.walks_biased(csr.rowptr, csr.col, n, starts, length, count[0], *form)

    def block_ms(run, k):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(k):
            last = run()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / k, last

    forms = ["first_order"] + BIASED_PQ
    label = lambda f: f if isinstance(f, str) else "biased_p%g_q%g" % f
    for f in forms:
        block_ms(lambda: launch(f), warmup)
    times = {label(f): [] for f in forms}
    for _ in range(reps):
        for f in forms:
            times[label(f)].append(block_ms(lambda: launch(f), steps)[0])

    # the exact pass's share, and the launch against the restatement at this size
    rowptr, col = csr.rowptr.cpu().numpy().astype(np.int64), csr.col.cpu().numpy().astype(np.int64)
    starts = batches[0]
    exact = {}
    for pq in BIASED_PQ:
        want, hits = restatement.walks_biased_ref(rowptr, col, n, starts.cpu().numpy(), length, 7, *pq)
        got = node2vec.walks_biased(csr.rowptr, csr.col, n, starts, length, 7, *pq).cpu().numpy()
        exact[label(pq)] = {"steps": int(starts.numel() * length), "reached_the_exact_pass": int(hits),
                            "share": hits / float(starts.numel() * length), "launch_equals_restatement": bool(np.array_equal(got, want))}

    # the full training step
    models = {"first_order": first, label(BIASED_STEP_PQ): second}
    step_batches = [order[lo:lo + BATCH] for lo in range(0, n - BATCH + 1, BATCH)]

    def step(m):
        count[0] += 1
        return m.step(step_batches[count[0] % len(step_batches)], count[0])

    step_times, last_loss = {k: [] for k in models}, {}
    for k, m in models.items():
        block_ms(lambda: step(m), warmup)
    for _ in range(reps):
        for k, m in models.items():
            ms, loss = block_ms(lambda: step(m), steps)
            assert bool(torch.isfinite(loss)), k
            step_times[k].append(ms)
            last_loss[k] = float(loss)
    faulthandler.cancel_dump_traceback_later()
    deg = np.diff(rowptr)
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"N": n, "E": int(ei.shape[1]), "max_out_degree": int(deg.max()), "mean_out_degree": float(deg.mean()),
            "walk_rows": int(starts.numel()), "walk_length": length, "launches_per_block": steps, "warmup_launches": warmup, "reps": reps,
            "walk_launch_ms": {k: stat(v) for k, v in times.items()},
            "walk_launch_over_first_order": {k: med[k] / med["first_order"] for k in med if k != "first_order"},
            "exact_pass": exact,
            "step_ms": {k: stat(v) for k, v in step_times.items()},
            "step_over_first_order": float(np.median(step_times[label(BIASED_STEP_PQ)]) / np.median(step_times["first_order"])),
            "last_loss": last_loss, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="pubmed,flickr")
    ap.add_argument("--steps", type=int, default=200, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=20, help="steps per form before the first timed block")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds one graph's run may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=("step", "biased"), default="step",
                    help="step: the training step (profiles/node2vec_times.json); biased: the second-order walk launch beside the "
                         "first-order one, and the step on biased walks (profiles/node2vec_biased_times.json)")
    ap.add_argument("--gpu-run", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.gpu_run:
        run = biased_run if args.leg == "biased" else gpu_run
        print(json.dumps(run(args.gpu_run, args.steps, args.warmup, args.reps, args.timeout)))
        return
    res = {}
    for name in args.graphs.split(","):
        child = subprocess.run(["timeout", "-k", "10", str(args.timeout + 20), sys.executable, os.path.abspath(__file__), "--gpu-run", name, "--leg", args.leg,
                                "--steps", str(args.steps), "--warmup", str(args.warmup), "--reps", str(args.reps),
                                "--timeout", str(args.timeout)], stdout=subprocess.PIPE, text=True)
        if child.returncode != 0:                        # a fault, an abort or the time limit: nothing more is started
            raise SystemExit(f"{name}: the GPU run ended with status {child.returncode}; stopping")
        res[name] = json.loads(child.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
