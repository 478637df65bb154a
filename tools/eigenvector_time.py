#!/usr/bin/env python3
"""Time engine.eigenvector_centrality (device edge_index -> host float64 scores, utils.py:44-48 nx.eigenvector_centrality_numpy)
on the Flickr-shaped graph and on R-MAT-22 (configs[4]'s graph): the whole call, the iteration count, the time of one
iteration (three launches: a run of iterations that never meets the stop test, between two events), the longest row and the
number of rows on the wave-per-row path.  Beside it the host path on the graphs named by --host: SciPy's ARPACK call as NetworkX
makes it, and -- where NetworkX 3 accepts the graph at all, i.e. on the largest strong component -- building the DiGraph and
nx.eigenvector_centrality_numpy.  Prints one JSON object; --out FILE also writes it there (DESIGN §7n:
profiles/eigenvector_times.json)."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphpope_amd import _lib, engine, synth  # noqa: E402

with open(os.path.join(ROOT, "graphpope_amd", "csrc", "eigenvector.hip")) as _f:      # the kernel's own split length
    WAVE_ROW = int(re.search(r"constexpr int EIG_WAVE_ROW = (\d+);", _f.read()).group(1))


def per_iteration_us(eid, n, iterations):
    """Mean time of one iteration on the device: `iterations` of them enqueued at once with a stop test that cannot pass."""
    lib = _lib.load()
    dev = eid.device
    t = engine.build_csr_canonical(eid.flip(0).contiguous(), n)
    x = torch.as_tensor(np.full(n, 1.0 / np.sqrt(n)), device=dev)
    control = torch.zeros(4, dtype=torch.int64, device=dev)
    scratch = torch.empty(lib.pope_eigenvector_scratch_bytes(n), dtype=torch.uint8, device=dev)

    def run(k):
        _lib.check(lib.pope_eigenvector_iterate(_lib.ptr(t.rowptr), _lib.ptr(t.col), n, _lib.ptr(x), _lib.ptr(scratch), scratch.numel(),
                                                k, 1e-300, _lib.ptr(control), engine._stream()))
    run(8)
    torch.cuda.synchronize()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    run(iterations)
    end.record()
    torch.cuda.synchronize()
    assert int(control.cpu()[3]) == 0
    return 1e3 * beg.elapsed_time(end) / iterations


def iterations_of(eid, n):
    """The iteration count of the call, read from a control block of our own."""
    lib = _lib.load()
    t = engine.build_csr_canonical(eid.flip(0).contiguous(), n)
    x = torch.as_tensor(np.full(n, 1.0 / np.sqrt(n)), device=eid.device)
    control = torch.zeros(4, dtype=torch.int64, device=eid.device)
    scratch = torch.empty(lib.pope_eigenvector_scratch_bytes(n), dtype=torch.uint8, device=eid.device)
    for _ in range(1250):
        _lib.check(lib.pope_eigenvector_iterate(_lib.ptr(t.rowptr), _lib.ptr(t.col), n, _lib.ptr(x), _lib.ptr(scratch), scratch.numel(),
                                                8, 1e-13, _lib.ptr(control), engine._stream()))
        state = control.cpu().numpy()
        if state[3]:
            return int(state[0]), float(state[1:2].view(np.float64)[0])
    raise SystemExit("no convergence")


def host_times(ei, n, networkx_too):
    import scipy.sparse as sp
    import scipy.sparse.linalg
    res = {}
    t0 = time.perf_counter()
    key = np.unique(ei[0] * n + ei[1])
    m = sp.csr_matrix((np.ones(len(key)), (key // n, key % n)), shape=(n, n))
    _, vec = scipy.sparse.linalg.eigs(m.T, k=1, which="LR", maxiter=50, tol=0)
    res["scipy_arpack_whole_graph_s"] = time.perf_counter() - t0
    if networkx_too:
        import networkx as nx
        _, label = sp.csgraph.connected_components(m, directed=True, connection="strong")
        big = np.flatnonzero(label == np.bincount(label).argmax())
        inside = np.isin(ei[0], big) & np.isin(ei[1], big)
        relabel = np.full(n, -1, dtype=np.int64)
        relabel[big] = np.arange(len(big))
        sub = relabel[ei[:, inside]]
        t0 = time.perf_counter()
        g = nx.DiGraph()
        g.add_nodes_from(range(len(big)))
        g.add_edges_from(zip(sub[0].tolist(), sub[1].tolist()))
        t1 = time.perf_counter()
        nx.eigenvector_centrality_numpy(g)
        res.update({"largest_strong_component_nodes": int(len(big)), "networkx_digraph_build_s": t1 - t0,
                    "networkx_call_s": time.perf_counter() - t1})
    return res


def run(ei, n, reps, warm, iters, host, networkx_too):
    eid = torch.as_tensor(ei, device=engine.require_gpu())
    for _ in range(warm):
        engine.eigenvector_centrality(eid, n)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        engine.eigenvector_centrality(eid, n)                        # CSR build, the loop, the copy of the scores to the host
        times.append(time.perf_counter() - t0)
    rows = np.bincount(ei[1], minlength=n)
    its, lam = iterations_of(eid, n)
    res = {"N": n, "E": int(ei.shape[1]), "reps": reps, "ms_min": 1e3 * min(times), "ms_median": 1e3 * float(np.median(times)),
           "ms_max": 1e3 * max(times), "iterations": its, "lambda": lam, "us_per_iteration": per_iteration_us(eid, n, iters),
           "launches_per_iteration": 3, "max_row": int(rows.max()), "rows_on_wave_path": int((rows >= WAVE_ROW).sum()),
           "wave_row_threshold": WAVE_ROW}
    if host:
        res["host"] = host_times(ei, n, networkx_too)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="flickr,rmat22")
    ap.add_argument("--host", default="flickr", help="graphs on which the host path is timed too (comma-separated, '' for none)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=200, help="length of the timed run of iterations")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    host = set(filter(None, args.host.split(",")))
    for g in args.graphs.split(","):
        if g == "flickr":
            ei, n = synth.flickr_like()
        elif g == "pubmed":
            ei, n = synth.pubmed_like()
        elif g == "rmat22":
            ei, n = synth.rmat(22, edge_factor=8, seed=1)
        else:
            raise SystemExit(f"unknown graph {g!r}")
        res[g] = run(ei, n, args.reps, args.warmup, args.iterations, g in host, n < 1_000_000)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
