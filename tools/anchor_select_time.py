#!/usr/bin/env python3
"""Time engine.score_anchors (utils.py:29-30 and the same two lines of every score method: ascending stable sort of the float64
scores, last K) at N = 89 250 with K = 256 (Flickr-sized) and N = 2^22 with K = 512 (R-MAT-22-sized), on two score vectors each:
all distinct, and clustering-like (about 60 % exactly 0.0, 10 % exactly 1.0, the rest spread between).  Per case: the host line
np.argsort(score, kind="stable")[-K:].tolist() in the same process; score_anchors from a host array with the upload included and
from a device tensor (host clock around a call that ends in the read-back of the K ids); pope_topk_f64 alone between two events.
Warm-up first, median of --reps calls (at least 20).  Checks that every path returns the same list.  Prints one JSON object;
--out FILE also writes it there (profiles/anchor_select_times.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphpope_amd import _lib, engine  # noqa: E402


def host_line(score, k):
    """What sample_anchor_nodes ran on the host for the five score methods."""
    order = np.argsort(score, kind="stable")
    return order[-k:].tolist()


def score_vectors(n, seed):
    rs = np.random.RandomState(seed)
    yield "all_distinct", rs.permutation(n).astype(np.float64) / n
    u = rs.rand(n)
    x = rs.randint(1, 64, n) / rs.randint(64, 4096, n).astype(np.float64)     # ratios of small integers, repeated values included
    x[u < 0.6] = 0.0
    x[u >= 0.9] = 1.0
    yield "clustering_like", x


def stats(times):
    return {"ms_min": 1e3 * min(times), "ms_median": 1e3 * float(np.median(times)), "ms_max": 1e3 * max(times)}


def wall(fn, reps, warm, sync=True):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                                     # ends in the read-back of the K ids (or never leaves the host)
        times.append(time.perf_counter() - t0)
    return stats(times)


def between_events(fn, reps, warm):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        beg.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(1e-3 * beg.elapsed_time(end))
    return stats(times)


def run(score, k, reps, warm, host_reps):
    lib = _lib.load()
    dev = engine.require_gpu()
    n = int(score.shape[0])
    score_dev = torch.as_tensor(score, device=dev)
    res = {"N": n, "K": k, "reps": reps, "warmup": warm, "zeros": float((score == 0.0).mean()), "ones": float((score == 1.0).mean()),
           "distinct_values": int(len(np.unique(score)))}
    res["host_line"] = dict(wall(lambda: host_line(score, k), host_reps, 1, sync=False), reps=host_reps)
    res["host_array_upload_included"] = wall(lambda: engine.score_anchors(score, k), reps, warm)
    res["device_tensor"] = wall(lambda: engine.score_anchors(score_dev, k), reps, warm)
    out = torch.empty(k, dtype=torch.int64, device=dev)
    scratch = torch.empty(lib.pope_topk_f64_scratch_bytes(n, k), dtype=torch.uint8, device=dev)
    res["select"] = between_events(
        lambda: _lib.check(lib.pope_topk_f64(_lib.ptr(score_dev), n, k, _lib.ptr(out), None, _lib.ptr(scratch), scratch.numel(),
                                             engine._stream())), reps, warm)
    res["select_scratch_bytes"] = int(scratch.numel())
    res["select_launches"] = 15                                  # one memset, thirteen passes, one sort
    res["score_bytes"] = 8 * n
    want = host_line(score, k)
    res["same_list"] = engine.score_anchors(score, k) == want and engine.score_anchors(score_dev, k) == want and out.cpu().tolist() == want
    if not res["same_list"]:
        raise SystemExit(f"device and host paths disagree on N = {n}, K = {k}")
    res["host_line_over_host_array"] = res["host_line"]["ms_median"] / res["host_array_upload_included"]["ms_median"]
    res["host_line_over_device_tensor"] = res["host_line"]["ms_median"] / res["device_tensor"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="flickr,rmat22")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps: at least 20")
    res = {}
    for size in args.sizes.split(","):
        if size == "flickr":
            n, k, host_reps = 89250, 256, 20
        elif size == "rmat22":
            n, k, host_reps = 1 << 22, 512, 20
        else:
            raise SystemExit(f"unknown size {size!r}")
        for name, score in score_vectors(n, seed=n % 1000):
            res[f"{size}_{name}"] = run(score, k, args.reps, args.warmup, host_reps)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
