#!/usr/bin/env python3
"""Time engine.degree_anchors (utils.py:38-42: nx.degree_centrality, ascending stable sort, last K) on the Flickr-shaped graph
(K = 256) and on R-MAT-22 (configs[4]'s graph, K = 512): the whole call from a device-resident edge_index and from a host tensor
with the upload included (host clock around a call that ends in the read-back of the K ids; warm-up first, median of --reps
calls), the canonical CSR build, the degree launch and the select each between two events, and the host expression
sample_anchor_nodes keeps for machines without a GPU, in the same process.  Checks that both paths return the same list.
Prints one JSON object; --out FILE also writes it there (profiles/degree_times.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphpope_amd import _lib, engine, synth  # noqa: E402


def host_expression(ei, n, k):
    """The degree branch of sample_anchor_nodes on a machine without a GPU (edge_index already a NumPy array)."""
    pairs = np.unique(ei[0] * n + ei[1])
    deg = np.bincount(pairs // n, minlength=n) + np.bincount(pairs % n, minlength=n)
    return np.argsort(deg, kind="stable")[-k:].tolist()


def stats(times):
    return {"ms_min": 1e3 * min(times), "ms_median": 1e3 * float(np.median(times)), "ms_max": 1e3 * max(times)}


def wall(fn, reps, warm):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                                     # ends in the read-back of the K ids
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


def run(ei, n, k, reps, warm, host_reps):
    lib = _lib.load()
    dev = engine.require_gpu()
    ei_host = torch.as_tensor(ei)
    eid = ei_host.to(dev)
    res = {"N": n, "E": int(ei.shape[1]), "K": k, "reps": reps, "warmup": warm}
    res["device_edge_index"] = wall(lambda: engine.degree_anchors(eid, n, k), reps, warm)
    res["host_edge_index_upload_included"] = wall(
        lambda: engine.degree_anchors(engine.stage_to_device(ei_host, dev).to(torch.int64), n, k), reps, warm)
    # the three device steps, each between two events (the CSR build synchronises once inside: its index check)
    res["csr_build_canonical"] = between_events(lambda: engine.build_csr_canonical(eid, n), reps, warm)
    csr = engine.build_csr_canonical(eid, n)
    deg = torch.empty(n, dtype=torch.int64, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    res["degree_launches"] = between_events(
        lambda: _lib.check(lib.pope_degree_counts(_lib.ptr(csr.rowptr), _lib.ptr(csr.col), _lib.ptr(csr.erow), n, _lib.ptr(deg),
                                                  _lib.ptr(keys), engine._stream())), reps, warm)
    out = torch.empty(k, dtype=torch.int64, device=dev)
    scratch = torch.empty(lib.pope_topk_scratch_bytes(n, k), dtype=torch.uint8, device=dev)
    res["select"] = between_events(
        lambda: _lib.check(lib.pope_topk_u64(_lib.ptr(keys), n, k, _lib.ptr(out), _lib.ptr(scratch), scratch.numel(), engine._stream())),
        reps, warm)
    res["select_scratch_bytes"] = int(scratch.numel())
    res["select_launches"] = 10
    got = engine.degree_anchors(eid, n, k)
    times = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        want = host_expression(ei, n, k)
        times.append(time.perf_counter() - t0)
    res["host_expression"] = dict(stats(times), reps=host_reps)
    res["same_list"] = got == want and engine.degree_anchors(engine.stage_to_device(ei_host, dev).to(torch.int64), n, k) == want
    if not res["same_list"]:
        raise SystemExit(f"device and host paths disagree on N = {n}, K = {k}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="flickr,rmat22")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    for g in args.graphs.split(","):
        if g == "flickr":
            (ei, n), k, host_reps = synth.flickr_like(), 256, 5
        elif g == "rmat22":
            (ei, n), k, host_reps = synth.rmat(22, edge_factor=8, seed=1), 512, 1
        else:
            raise SystemExit(f"unknown graph {g!r}")
        res[g] = run(ei, n, k, args.reps, args.warmup, host_reps)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
