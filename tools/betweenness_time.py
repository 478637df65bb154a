#!/usr/bin/env python3
"""Time engine.betweenness_centrality (device edge_index -> host float64 scores, utils.py:32-36 nx.betweenness_centrality) on
the PubMed-shaped and the Flickr-shaped graph: seconds of the full run, batch size and workspace bytes used, the identity
check of the result against the multi-source BFS kernel (sum_v bc[v] = sum over reachable ordered pairs of d(s, t) - 1), and
NetworkX's time for the same graph extrapolated from a timed sample of sources on this host.
Every graph's GPU run is a child process of its own under a time limit, and the first one that fails ends the run.
Prints one JSON object; --out FILE also writes it there (profiles/betweenness_times.json)."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphpope_amd import synth  # noqa: E402


def graph(name):
    if name == "flickr":
        return synth.flickr_like()
    if name == "pubmed":
        return synth.pubmed_like()
    raise SystemExit(f"unknown graph {name!r}")


def gpu_run(name):
    """The child: one full run on the GPU, and the exact integer it must sum to from engine.bfs + engine.column_stats."""
    import torch
    from graphpope_amd import engine
    ei, n = graph(name)
    dev = engine.require_gpu()
    eid = torch.as_tensor(ei, device=dev)
    ring = np.stack([np.arange(64), (np.arange(64) + 1) % 64]).astype(np.int64)
    engine.betweenness_centrality(torch.as_tensor(ring, device=dev), 64)          # library, context and allocator warm
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bc = engine.betweenness_centrality(eid, n, normalized=False, stats=stats)
    seconds = time.perf_counter() - t0
    csr = engine.build_csr(torch.as_tensor(np.ascontiguousarray(ei[::-1]), device=dev), n)
    want = 0
    for lo in range(0, n, 256):
        hop_sum, reach = engine.column_stats(engine.bfs(csr, np.arange(lo, min(lo + 256, n))))
        want += int(hop_sum.sum()) - int((reach - 1).sum())
    got = math.fsum(bc.tolist())
    max_in = int(np.bincount(np.unique(ei[0] * n + ei[1]) % n, minlength=n).max())
    return {"N": n, "E": int(ei.shape[1]), "seconds": seconds, "batch": stats["batch"], "workspace_bytes": stats["workspace_bytes"],
            "sources_per_second": n / seconds, "sum_bc": got, "bfs_identity": want, "identity_relative_difference": abs(got - want) / want,
            "identity_bound": 4 * (n + max_in) * 2.0 ** -53, "max_in_degree": max_in, "device": torch.cuda.get_device_name(0)}


def networkx_sample(name, k):
    """NetworkX on this host: k sampled sources timed, the full run extrapolated (N / k times that)."""
    import networkx as nx
    ei, n = graph(name)
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(ei[0].tolist(), ei[1].tolist()))
    t0 = time.perf_counter()
    nx.betweenness_centrality(g, k=k, seed=0)
    seconds = time.perf_counter() - t0
    return {"networkx_sampled_sources": k, "networkx_sample_seconds": seconds, "networkx_extrapolated_seconds": seconds * n / k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="pubmed,flickr")
    ap.add_argument("--sample", type=int, default=8, help="sources NetworkX is timed on")
    ap.add_argument("--timeout", type=int, default=300, help="seconds one graph's GPU run may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--gpu-run", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.gpu_run:
        print(json.dumps(gpu_run(args.gpu_run)))
        return
    res = {}
    for name in args.graphs.split(","):
        child = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--gpu-run", name],
                               stdout=subprocess.PIPE, text=True)
        if child.returncode != 0:                        # a fault, an abort or the time limit: nothing more is started
            raise SystemExit(f"{name}: the GPU run ended with status {child.returncode}; stopping")
        res[name] = json.loads(child.stdout.strip().splitlines()[-1])
        res[name].update(networkx_sample(name, args.sample))
        res[name]["speedup_over_networkx_extrapolated"] = res[name]["networkx_extrapolated_seconds"] / res[name]["seconds"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
