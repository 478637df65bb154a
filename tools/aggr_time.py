#!/usr/bin/env python3
"""Time the aggregation half of SAGEConv(aggr='add' | 'max') (csrc/aggregate.hip) against the mean's kernels and against stock torch ops,
and the replayed training step under the three aggregators.  Everything in this one process on one GPU:

    gather, layer-0 shape    40 300 destinations x fan-out 10 x 756 columns, sources among 85 000 rows
        mean                     sage_gather_mean over the materialised source rows (that entry point has no indexed mode)
        add / max / max_arg      sage_aggregate_forward over the same rows (max_arg: arg recorded as well)
        add_indexed / max_indexed    the same block read through n_id from an 89 250-row feature matrix, x_dst written
        torch_add / torch_max    index_select + scatter_reduce('sum' | 'amax'), forward only (layer 0 takes no input gradient)
    gather, hidden shape     1 550 destinations x fan-out 25 x 256 columns, 40 300 sources: mean, add, max, max_arg, torch_add, torch_max
    backward, hidden shape   grad_agg [1 550, 256] -> grad_x [40 300, 256]
        mean_det                 sage_scatter_mean_det (index build + k_scatter_sum_det)
        add / max                sage_aggregate_backward (the same index build + k_scatter_ordered)
        torch_add / torch_max    autograd's backward pass of index_select + scatter_reduce
    step                     SAGE(756, 7, 256, 3), batch 1 550, fan-out [25, 10] sampled on the device, Flickr-shaped synthetic graph
        replayed_mean / _add / _max      graphpope_amd.train.SageTrainStep, captured and replayed, epoch mode
        torch_mean / _add / _max         the same model written in stock torch ops (index_select + scatter_reduce, F.linear, BatchNorm1d,
                                         relu_, F.dropout, F.cross_entropy, torch.optim.Adam) on ONE pre-sampled batch, eager

The time between two HIP events around a block of --steps calls, divided by the calls; --reps blocks per form (five), the forms of a
group taken in turns so that drift of the machine lands on all alike; median / min / max per form.  Results of the library's forms are
compared with the torch forms first.  Prints one JSON object; --out FILE also writes it there (profiles/aggr_times.json).  The run ends
itself after --time-limit seconds; run it under `timeout` too."""
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
from graphpope_amd import _lib, engine, sage, synth  # noqa: E402

AGGR = _lib.AGGR
P = _lib.ptr
LAYER0 = dict(n_dst=40300, fanout=10, n_src=85000, c=756, rows=89250)
HIDDEN = dict(n_dst=1550, fanout=25, n_src=40300, c=256, rows=40300)
C_IN, WIDTH, LAYERS, CLASSES, BATCH, SIZES = 756, 256, 3, 7, 1550, (25, 10)


def events_us(fn, k):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(k):
        fn()
    t1.record()
    t1.synchronize()
    return 1e3 * t0.elapsed_time(t1) / k


def stats(ts):
    return {"median": float(np.median(ts)), "min": min(ts), "max": max(ts), "all": ts}


def time_group(forms, args):
    for fn in forms.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in forms}
    for _ in range(args.reps):
        for k, fn in forms.items():
            times[k].append(events_us(fn, args.steps))
    return {k: stats(ts) for k, ts in times.items()}


class Block:
    """A fan-out block with its rows, on the device, and every form of its two halves as a callable over buffers allocated once."""

    def __init__(self, dev, n_dst, fanout, n_src, c, rows, seed=0):
        self.dev, self.n_dst, self.n_src, self.c, self.rows, self.lib = dev, n_dst, n_src, c, rows, _lib.load()
        g = torch.Generator().manual_seed(seed)
        self.nnz = n_dst * fanout
        self.rowptr = (torch.arange(n_dst + 1, dtype=torch.int32) * fanout).to(dev)
        self.col = torch.randint(0, n_src, (self.nnz,), generator=g, dtype=torch.int32).to(dev)
        self.feats = torch.randn(rows, c, generator=g).to(dev)
        self.n_id = torch.randperm(rows, generator=g)[:n_src].to(dev)
        self.x = self.feats.index_select(0, self.n_id) if rows != n_src else self.feats      # the materialised source rows
        if rows == n_src:
            self.n_id = None
        self.agg = torch.empty((n_dst, c), dtype=torch.float32, device=dev)
        self.arg = torch.empty((n_dst, c), dtype=torch.int32, device=dev)
        self.x_dst = torch.empty((n_dst, c), dtype=torch.float32, device=dev)
        self.row64 = torch.arange(n_dst, device=dev).repeat_interleave(fanout)
        self.col64 = self.col.long()
        self.index = self.row64[:, None].expand(-1, c)

    def mean(self):
        _lib.check(self.lib.sage_gather_mean(P(self.rowptr), P(self.col), self.n_src, self.n_dst, self.nnz, P(self.x), self.c, P(self.agg), sage._stream()))
        return self.agg

    def gather(self, aggr, arg=False, indexed=False):
        x, n_id, x_dst = (self.feats, self.n_id, self.x_dst) if indexed else (self.x, None, None)

        def call():
            _lib.check(self.lib.sage_aggregate_forward(P(self.rowptr), P(self.col), P(n_id), self.n_src, self.n_dst, self.nnz, P(x), x.shape[0], self.c,
                                                       AGGR[aggr], P(self.agg), P(self.arg if arg else None), P(x_dst), None, sage._stream()))
            return self.agg
        return call

    def torch_gather(self, aggr, x=None):
        x = self.x if x is None else x
        out = torch.zeros((self.n_dst, self.c), dtype=torch.float32, device=self.dev)
        return out.scatter_reduce(0, self.index, x.index_select(0, self.col64), "sum" if aggr == "add" else "amax", include_self=False)

    def backward_forms(self):
        g = torch.randn(self.n_dst, self.c, generator=torch.Generator().manual_seed(1)).to(self.dev)
        gx = torch.zeros((self.n_src, self.c), dtype=torch.float32, device=self.dev)
        nbytes = self.lib.sage_aggregate_backward_scratch_size(self.n_src, self.n_dst, self.nnz)
        assert nbytes == self.lib.sage_scatter_mean_det_scratch_bytes(self.n_src, self.n_dst, self.nnz)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        self.gather("max", arg=True)()
        arg = self.arg.clone()
        head = (P(self.rowptr), P(self.col), self.n_src, self.n_dst, self.nnz)

        def mean_det():
            _lib.check(self.lib.sage_scatter_mean_det(*head, P(g), self.c, P(gx), P(scratch), nbytes, None, sage._stream()))
            return gx

        def ordered(aggr):
            def call():
                _lib.check(self.lib.sage_aggregate_backward(*head, P(arg if aggr == "max" else None), P(g), self.c, AGGR[aggr], P(gx), P(scratch), nbytes,
                                                            None, sage._stream()))
                return gx
            return call

        def torch_backward(aggr):
            x = self.x.detach().clone().requires_grad_(True)
            out = self.torch_gather(aggr, x)                           # the graph is built once; the timed call is the backward pass alone

            def call():
                return torch.autograd.grad(out, x, g, retain_graph=True)[0]
            return call
        return {"mean_det": mean_det, "add": ordered("add"), "max": ordered("max"), "torch_add": torch_backward("add"),
                "torch_max": torch_backward("max")}, g, gx


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-30))


def gather_group(blk, indexed):
    forms = {"mean": blk.mean, "add": blk.gather("add"), "max": blk.gather("max"), "max_arg": blk.gather("max", arg=True)}
    if indexed:
        forms.update({"add_indexed": blk.gather("add", indexed=True), "max_indexed": blk.gather("max", indexed=True)})
    forms.update({"torch_add": lambda: blk.torch_gather("add"), "torch_max": lambda: blk.torch_gather("max")})
    agree = {"add_vs_torch": rel(forms["add"]().clone(), forms["torch_add"]()), "max_vs_torch": rel(forms["max"]().clone(), forms["torch_max"]())}
    if indexed:
        agree["add_indexed_vs_add"] = rel(forms["add_indexed"]().clone(), forms["add"]().clone())
        agree["x_dst"] = rel(blk.x_dst, blk.x[:blk.n_dst])
    assert max(agree.values()) < 1e-5, agree
    return forms, agree


class TorchSage(torch.nn.Module):
    """The model of graphpope_amd.sage.SAGE in stock torch ops, the depth quirk included (one conv per sampled block)."""

    def __init__(self, aggr):
        super().__init__()
        widths = [C_IN] + [WIDTH] * (LAYERS - 1) + [CLASSES]
        self.aggr = aggr
        self.lin_l = torch.nn.ModuleList(torch.nn.Linear(a, b) for a, b in zip(widths, widths[1:]))
        self.lin_r = torch.nn.ModuleList(torch.nn.Linear(a, b, bias=False) for a, b in zip(widths, widths[1:]))
        self.bns = torch.nn.ModuleList(torch.nn.BatchNorm1d(WIDTH) for _ in range(LAYERS - 1))

    def forward(self, x, blocks):
        for i, (row, col, n_dst, inv_deg) in enumerate(blocks):
            out = torch.zeros((n_dst, x.shape[1]), dtype=x.dtype, device=x.device)
            g = x.index_select(0, col)
            index = row[:, None].expand(-1, x.shape[1])
            if self.aggr == "max":
                agg = out.scatter_reduce(0, index, g, "amax", include_self=False)
            else:
                agg = out.scatter_reduce(0, index, g, "sum", include_self=False)
                if self.aggr == "mean":
                    agg = agg * inv_deg[:, None]
            x = self.lin_l[i](agg) + self.lin_r[i](x[:n_dst])
            if i < len(blocks) - 1:
                x = F.dropout(self.bns[i](x).relu_(), 0.5, self.training)
        return x


def step_group(dev, args):
    ei, n = synth.flickr_like(seed=1)
    from graphpope_amd.optim import Adam
    from graphpope_amd.sampler import NeighborSampler
    from graphpope_amd.train import SageTrainStep
    feats = torch.rand(n, C_IN, generator=torch.Generator().manual_seed(0)).to(dev)
    csr = engine.build_csr(torch.as_tensor(ei, device=dev), n)
    sampler = NeighborSampler(csr.rowptr, csr.col, n, SIZES)
    perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    labels = torch.randint(0, CLASSES, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    forms, keep = {}, []
    for aggr in ("mean", "add", "max"):
        torch.manual_seed(0)
        model = sage.SAGE(C_IN, CLASSES, WIDTH, LAYERS, aggr=aggr).to(dev)
        opt = Adam(model.parameters(), lr=0.01, max_grad_norm=0.5)
        st = SageTrainStep(model, opt, feats, BATCH, sampler=sampler, graph=True)
        keep.append((model, opt, st))

        def step(st=st):
            if st.batches_left() < 1:
                st.set_epoch(perm, labels)
            return st.step_epoch()
        st.set_epoch(perm, labels)
        forms["replayed_" + aggr] = step
    # one pre-sampled batch for the stock-torch model
    rowptr, col = csr.rowptr.cpu().numpy().astype(np.int64), csr.col.cpu().numpy().astype(np.int64)[:int(csr.num_edges)]
    n_id, adjs = sage.sample_batch(rowptr, col, np.arange(BATCH, dtype=np.int64), sizes=SIZES, rng=np.random.default_rng(0))
    n_id_dev, y = torch.as_tensor(n_id, device=dev), labels[:BATCH].contiguous()
    blocks = []
    for a in adjs:
        deg = np.diff(a.rowptr.numpy())
        blocks.append((torch.as_tensor(np.repeat(np.arange(a.n_dst), deg), device=dev), a.col.long().to(dev), a.n_dst,
                       torch.as_tensor(1.0 / np.maximum(deg, 1), dtype=torch.float32, device=dev)))
    shapes = [(a.n_dst, a.n_src, int(a.col.numel())) for a in adjs]
    for aggr in ("mean", "add", "max"):
        torch.manual_seed(0)
        tm = TorchSage(aggr).to(dev).train()
        topt = torch.optim.Adam(tm.parameters(), lr=0.01)
        keep.append((tm, topt))

        def tstep(tm=tm, topt=topt):
            topt.zero_grad(set_to_none=True)
            loss = F.cross_entropy(tm(feats.index_select(0, n_id_dev), blocks), y)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(tm.parameters(), 0.5)
            topt.step()
            return loss
        forms["torch_" + aggr] = tstep
    losses = {k: float(fn()) for k, fn in forms.items()}
    assert all(np.isfinite(v) for v in losses.values()), losses
    out = time_group(forms, args)
    return {"forms": out, "first_loss": losses, "graph": {"nodes": n, "edges": int(csr.num_edges)}, "torch_batch_blocks": shapes}


def spread_verdict(forms, new, old):
    a, b = forms[new], forms[old]
    spreads = (a["max"] - a["min"]) + (b["max"] - b["min"])
    return {"new": new, "against": old, "difference_us": a["median"] - b["median"], "two_spreads_us": spreads,
            "inside_the_spread": bool(abs(a["median"] - b["median"]) <= spreads), "ratio": a["median"] / b["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the training-step group")
    ap.add_argument("--time-limit", type=int, default=420, help="seconds after which the run ends itself")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.time_limit, exit=True)
    dev = engine.require_gpu()
    res = {"calls_per_block": args.steps, "warmup_calls": args.warmup, "reps": args.reps, "unit": "us per call, HIP events around a block",
           "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "groups": {}}
    for name, shape, indexed in (("gather_layer0", LAYER0, True), ("gather_hidden", HIDDEN, False)):
        blk = Block(dev, **shape)
        forms, agree = gather_group(blk, indexed)
        out = {"shape": shape, "max_relative_difference": agree, "forms": time_group(forms, args)}
        out["verdicts"] = [spread_verdict(out["forms"], k, "mean") for k in ("add", "max", "max_arg")]
        out["bytes_gathered"] = blk.nnz * blk.c * 4
        res["groups"][name] = out
        if name == "gather_hidden":
            forms, g, gx = blk.backward_forms()
            gx.zero_()
            want_add = forms["torch_add"]().clone()
            got_add = forms["add"]().clone()
            gx.zero_()
            want_max = forms["torch_max"]().clone()
            got_max = forms["max"]().clone()
            agree = {"add_vs_torch": rel(got_add, want_add), "max_vs_torch": rel(got_max, want_max)}
            assert max(agree.values()) < 1e-5, agree
            # (the timed calls add into the destination rows of grad_x again and again: zeroed between blocks by no one -- the values grow
            #  linearly and stay finite over the few hundred calls of a run; the time does not depend on them)
            out = {"shape": shape, "max_relative_difference": agree, "forms": time_group(forms, args)}
            out["verdicts"] = [spread_verdict(out["forms"], k, "mean_det") for k in ("add", "max")]
            res["groups"]["backward_hidden"] = out
        del blk
        torch.cuda.empty_cache()
    if not args.no_step:
        out = step_group(dev, args)
        out["verdicts"] = [spread_verdict(out["forms"], "replayed_" + k, "replayed_mean") for k in ("add", "max")]
        out["verdicts"] += [spread_verdict(out["forms"], "replayed_" + k, "torch_" + k) for k in ("mean", "add", "max")]
        res["groups"]["step"] = out
    faulthandler.cancel_dump_traceback_later()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
