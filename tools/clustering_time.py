#!/usr/bin/env python3
"""Time engine.clustering_coefficient (device edge_index -> host float64 scores, utils.py:56-60 nx.clustering) on the
Flickr-shaped graph and on R-MAT-22 (configs[4]'s graph), and count the work the triangle kernel does on each: the oriented
pairs, the largest oriented row, the probes sum over oriented (i, j) of |N+(j)|, and the 64-bit atomics it may issue.
Prints one JSON object; --out FILE also writes it there (profiles/clustering_times.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphpope_amd import engine, synth  # noqa: E402


def work_counts(ei, n, t):
    """Host-side counts of the oriented graph the kernel walks (order: distinct degree, then id)."""
    src, dst = ei[0], ei[1]
    keep = src != dst
    lo, hi = np.minimum(src[keep], dst[keep]), np.maximum(src[keep], dst[keep])
    pair = np.unique(lo * n + hi)
    a, b = pair // n, pair % n
    deg = np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
    a_first = (deg[a] < deg[b]) | ((deg[a] == deg[b]) & (a < b))
    tail, head = np.where(a_first, a, b), np.where(a_first, b, a)
    out = np.bincount(tail, minlength=n)
    inn = np.bincount(head, minlength=n)
    return {"pairs": int(len(pair)), "max_degree": int(deg.max()), "max_oriented_row": int(out.max()),
            "rows_over_1024": int((out > 1024).sum()), "probes": int((out.astype(np.int64) * inn).sum()),
            "atomic_bound": int(len(pair) + n), "sum_T_over_6": int(t.sum() // 6)}


def run(name, ei, n, reps, warm):
    eid = torch.as_tensor(ei, device=engine.require_gpu())
    for _ in range(warm):
        engine.clustering_coefficient(eid, n)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        engine.clustering_coefficient(eid, n)                     # ends with the copy of the counts to the host
        times.append(time.perf_counter() - t0)
    t, _, _ = engine.clustering_counts(eid, n)
    res = {"N": n, "E": int(ei.shape[1]), "reps": reps, "ms_min": 1e3 * min(times), "ms_median": 1e3 * float(np.median(times)),
           "ms_max": 1e3 * max(times)}
    res.update(work_counts(ei, n, t))
    res["probes_per_s_at_median"] = res["probes"] / (res["ms_median"] * 1e-3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="flickr,rmat22")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    for g in args.graphs.split(","):
        if g == "flickr":
            ei, n = synth.flickr_like()
        elif g == "pubmed":
            ei, n = synth.pubmed_like()
        elif g == "rmat22":
            ei, n = synth.rmat(22, edge_factor=8, seed=1)
        else:
            raise SystemExit(f"unknown graph {g!r}")
        res[g] = run(g, ei, n, args.reps, args.warmup)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
