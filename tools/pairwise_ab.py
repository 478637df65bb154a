#!/usr/bin/env python3
"""The `pairwise` leg of bench.py (configs[2]) with two builds of the library, alternating, each run in a process of its own (GPU box):
    python tools/pairwise_ab.py path/to/other/libgraphpope_hip.so [runs, default 7] > times.json
Prints one JSON object: per build the series of pairwise_ms_per_call (features + embedding) and pairwise_embedding_only_ms, their medians
and ranges.  "other" is the library given by path, "tree" the one this tree built."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import ctypes, json, sys
import torch                                   # before any other user of the HIP runtime is loaded
sys.path.insert(0, %r)
from graphpope_amd import _lib
if sys.argv[1] != "tree":
    _lib.LIB_PATH = sys.argv[1]
    probe = ctypes.CDLL(_lib.LIB_PATH)
    for name in [s for s in _lib.SIGNATURES if not hasattr(probe, s)]:
        del _lib.SIGNATURES[name]
import bench
from graphpope_amd import engine, synth
dev = engine.require_gpu()
n = synth.FLICKR_N
x = torch.rand((n, 500), device=dev)
r = bench.pairwise_leg(n, synth.seeded_anchors(n, 256, 42), x, dev, steps=int(sys.argv[2]))
print(json.dumps({"pairwise_ms_per_call": r["ms_per_call"], "pairwise_embedding_only_ms": r["embedding_only_ms"]}))
''' % ROOT

if __name__ == "__main__":
    other, runs = os.path.abspath(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 7
    steps = 20                                                            # what bench.py gives the leg
    series = {"other": [], "tree": []}
    for rnd in range(runs):
        for build, lib in (("other", other), ("tree", "tree")):
            out = subprocess.run([sys.executable, "-c", CHILD, lib, str(steps)], capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                sys.exit("run %d of %s failed (%d): %s" % (rnd, build, out.returncode, out.stderr[-600:]))
            series[build].append(json.loads(out.stdout.strip().split("\n")[-1]))
            print(rnd, build, series[build][-1], file=sys.stderr, flush=True)
    result = {"workload": "bench.py pairwise_leg (configs[2]: N = 89 250, D = 128, K = 256, F = 500, euclidean, anchors by id), %d calls per run, "
                          "%d runs per build, alternating, one process each" % (steps, runs), "other_library": sys.argv[1]}
    for build, rows in series.items():
        for key in ("pairwise_ms_per_call", "pairwise_embedding_only_ms"):
            v = [r[key] for r in rows]
            result["%s_%s" % (build, key)] = {"runs": v, "median": float(np.median(v)), "min": min(v), "max": max(v)}
    print(json.dumps(result, indent=1))
