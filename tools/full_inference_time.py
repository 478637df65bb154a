#!/usr/bin/env python3
"""Time exact full-graph inference (SAGE.inference: sage_full_layer_forward, project-first) against the composition a user could already
write -- SAGEConv on the whole CSR as one block (aggregate-first), then bn_relu_dropout(training=False) -- on the Flickr-shaped and the
PubMed-shaped synthetic graphs, 500 + 256 input columns, 756 -> 256 -> 256, hops = 2.  Everything in this one process on one GPU:

    inference / composition                    both layers, as a user calls them (allocations included)
    inference_layer0 / composition_layer0      layer 0 alone: the call the keep rule of DESIGN.md 7t compares
    inference_layer1 / composition_layer1      layer 1 alone (conv without BatchNorm)

The time between two HIP events around a block of --steps calls, divided by the calls; --reps blocks per form (five), the forms taken
in turns so that drift of the machine lands on all alike; median / min / max per form.  The two paths' results are compared first.
Keep rule: the aggregate kernel stays if layer 0's median is below the composition's by more than the two spreads (max - min) together.

Per-launch times come from a kernel trace, which is a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir>/<graph>_layer<i> -- python3 tools/full_inference_time.py --trace <graph> <i>
and `--kernel-stats <dir>` folds the *_kernel_stats.csv files found there into the result: each launch's average, and the hub launches'
share of the layer (`--merge FILE` folds them into the JSON of an earlier timing run).  Without them the JSON says "not measured".  Prints one JSON object; --out FILE also writes it there
(profiles/full_inference_times.json).  The run ends itself after --time-limit seconds; run it under `timeout` too."""
import argparse
import csv
import ctypes
import faulthandler
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphpope_amd import _lib, engine, sage, synth  # noqa: E402

C_IN, HIDDEN, LAYERS, CLASSES, HOPS, CHUNK = 756, 256, 3, 7, 2, 512
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


class World:
    """One graph with its features, the model, and every form as a callable."""

    def __init__(self, name, dev, trace=False):
        ei, n = GRAPHS[name]()
        self.name, self.n, self.dev = name, n, dev
        g = torch.Generator().manual_seed(0)
        self.x = torch.rand(n, C_IN, generator=g).to(dev)
        self.csr = engine.build_csr(torch.as_tensor(ei).flip(0).contiguous().to(dev), n)
        self.nnz = int(self.csr.num_edges)
        self.block = sage.SampledAdj(self.csr.rowptr, self.csr.col[:self.nnz], n)      # the whole CSR as one "block"
        torch.manual_seed(0)
        self.model = sage.SAGE(C_IN, CLASSES, HIDDEN, LAYERS).to(dev).eval()
        with torch.no_grad():
            for bn in self.model.bns:                                                  # statistics a trained model would have
                bn.running_mean.uniform_(-0.5, 0.5)
                bn.running_var.uniform_(0.5, 2.0)
        self.deg = np.diff(self.csr.rowptr.cpu().numpy().astype(np.int64))
        self.lib = _lib.load()
        # layer 1's input (in a trace run random rows, so that no kernel of another layer or path gets into the statistics)
        self.h = torch.rand(n, HIDDEN, generator=g).to(dev) if trace else self.composition_layer0()
        self._raw = [self._raw_layer(0, self.x), self._raw_layer(1, self.h)]

    def inference(self):
        return self.model.inference(self.x, self.csr, hops=HOPS)

    def composition_layer0(self):
        m = self.model
        with torch.no_grad():
            return sage.bn_relu_dropout(m.convs[0](self.x, self.block), m.bns[0], m.dropout, training=False)

    def composition_layer1(self):
        with torch.no_grad():
            return self.model.convs[1](self.h, self.block)

    def composition(self):
        m = self.model
        with torch.no_grad():
            h = sage.bn_relu_dropout(m.convs[0](self.x, self.block), m.bns[0], m.dropout, training=False)
            return m.convs[1](h, self.block)

    def _raw_layer(self, i, x):
        """sage_full_layer_forward of layer i on buffers allocated once: the launches alone."""
        conv, bn = self.model.convs[i], (self.model.bns[i] if i < HOPS - 1 else None)
        c_in, c_out = conv.in_channels, conv.out_channels
        out = torch.empty((self.n, c_out), dtype=torch.float32, device=self.dev)
        nbytes = self.lib.sage_full_layer_scratch_size(self.n, self.nnz, c_in, c_out)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        norm = (None,) * 4 if bn is None else (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        p = _lib.ptr
        args = (p(self.csr.rowptr), p(self.csr.col), self.n, self.nnz, p(x), c_in, p(conv.lin_l.weight), p(conv.lin_l.bias), p(conv.lin_r.weight),
                c_out, *(p(t) for t in norm), float(bn.eps) if bn is not None else 0.0, p(out), p(scratch), nbytes)
        keep = (x, out, scratch)

        def call():
            _lib.check(self.lib.sage_full_layer_forward(*args, sage._stream()))
            return keep[1]
        return call

    def inference_layer0(self):
        return self._raw[0]()

    def inference_layer1(self):
        return self._raw[1]()

    def kernel_names(self, cus):
        names = []
        for c_in, bn in ((C_IN, 1), (HIDDEN, 0)):
            b = ctypes.create_string_buffer(384)
            _lib.check(self.lib.sage_full_layer_kernel_name(self.n, self.nnz, c_in, HIDDEN, bn, cus, 0, b, 384))
            names.append(b.value.decode())
        return names

    def degrees(self):
        d = self.deg
        hubs = d > CHUNK
        return {"nodes": int(self.n), "slots": int(d.sum()), "median": float(np.median(d)), "p99": float(np.percentile(d, 99)), "max": int(d.max()),
                "rows_longer_than_chunk": int(hubs.sum()), "share_of_slots_in_those_rows": float(d[hubs].sum() / max(d.sum(), 1)), "chunk": CHUNK}


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def fold_kernel_stats(directory, graph, layer):
    """{kernel: average us} of the trace of one layer, or None."""
    files = sorted(glob.glob(os.path.join(directory, f"{graph}_layer{layer}", "**", "*_kernel_stats.csv"), recursive=True))
    if not files:
        return None
    out = {}
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            short = name.split("pope::", 1)[-1].split("(", 1)[0]
            if short.startswith(("k_full_", "k_gemm")):
                out[short] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3}
    return out


def hub_share(launches):
    if not launches:
        return "not measured"
    total = sum(v["average_us"] for v in launches.values())
    hub = sum(v["average_us"] for k, v in launches.items() if k.startswith("k_full_hub_"))
    return hub / total if total else "not measured"


def trace(graph, layer, calls):
    dev = engine.require_gpu()
    w = World(graph, dev, trace=True)
    fn = w.inference_layer0 if layer == 0 else w.inference_layer1
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    print("traced", graph, "layer", layer, calls, "calls")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--graphs", default="flickr,pubmed")
    ap.add_argument("--time-limit", type=int, default=420, help="seconds after which the run ends itself")
    ap.add_argument("--kernel-stats", default=None, help="directory of <graph>_layer<i>/ kernel traces to fold in")
    ap.add_argument("--trace", nargs=2, metavar=("GRAPH", "LAYER"), default=None, help="only run one layer's call (for a kernel trace)")
    ap.add_argument("--merge", default=None, help="a JSON this tool wrote: fold --kernel-stats into it instead of timing again")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    faulthandler.dump_traceback_later(args.time_limit, exit=True)
    if args.trace:
        trace(args.trace[0], int(args.trace[1]), args.steps)
        return
    if args.merge:                                                 # the timings of an earlier run, the traces folded in now: needs no GPU
        faulthandler.cancel_dump_traceback_later()
        with open(args.merge) as f:
            return finish(json.load(f), args)
    dev = engine.require_gpu()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def stats(ts):
        return {"median": float(np.median(ts)), "min": min(ts), "max": max(ts), "all": ts}

    res = {"shape": {"in_channels": C_IN, "hidden": HIDDEN, "layers": LAYERS, "hops": HOPS, "widths": [C_IN, HIDDEN, HIDDEN]},
           "calls_per_block": args.steps, "warmup_calls": args.warmup, "reps": args.reps, "unit": "us per call, HIP events around a block",
           "device": torch.cuda.get_device_name(0), "compute_units": cus, "graphs": {}}
    for name in args.graphs.split(","):
        w = World(name, dev)
        agreement = {"inference_vs_composition": rel_err(w.inference(), w.composition()),
                     "layer0": rel_err(w.inference_layer0(), w.composition_layer0()), "layer1": rel_err(w.inference_layer1(), w.composition_layer1())}
        assert max(agreement.values()) < 1e-4, agreement
        forms = {k: getattr(w, k) for k in ("inference", "composition", "inference_layer0", "composition_layer0", "inference_layer1",
                                            "composition_layer1")}
        for fn in forms.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, fn in forms.items():
                times[k].append(events_us(fn, args.steps))
        out = {"degrees": w.degrees(), "max_relative_difference": agreement, "launch_lists": w.kernel_names(cus),
               "forms": {k: stats(ts) for k, ts in times.items()}}
        new, old = out["forms"]["inference_layer0"], out["forms"]["composition_layer0"]
        spreads = (new["max"] - new["min"]) + (old["max"] - old["min"])
        out["keep_rule"] = {"layer0_gain_us": old["median"] - new["median"], "two_spreads_us": spreads,
                            "aggregate_kernel_stays": bool(old["median"] - new["median"] > spreads),
                            "layer0_composition_over_inference": old["median"] / new["median"],
                            "both_layers_composition_over_inference": out["forms"]["composition"]["median"] / out["forms"]["inference"]["median"]}
        res["graphs"][name] = out
        del w
        torch.cuda.empty_cache()
    faulthandler.cancel_dump_traceback_later()
    finish(res, args)


def finish(res, args):
    """Fold the kernel traces in (per layer: each launch's average, the hub launches' share), print, write."""
    for name, out in res["graphs"].items():
        launches = [fold_kernel_stats(args.kernel_stats, name, i) if args.kernel_stats else None for i in range(HOPS)]
        out["launches"] = [ls if ls else "not measured" for ls in launches]
        out["hub_launches_share"] = [hub_share(ls) for ls in launches]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
