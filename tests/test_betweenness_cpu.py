"""Betweenness anchors (utils.py:32-36 nx.betweenness_centrality), the parts that need no GPU: the Python restatement of the
replay kernel -- NetworkX's additions in NetworkX's order, a row shared `lanes` slots at a time -- which is the kernel's
specification and what the GPU tests compare per-source rows with, and the C ABI's argument checks and scratch query."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_clustering_cpu import digraph, random_multigraph


@pytest.fixture(autouse=True)
def _clean_error_string():
    """The library's error string is per thread and outlives a test: the rejected calls below would leave theirs to whichever
    test runs next in this process (test_abi reads it as empty).  A successful host-only call clears it."""
    yield
    from graphpope_amd import _lib
    buf = ctypes.create_string_buffer(64)
    _lib.check(_lib.load().pope_level_kernel_name(89250, 256, buf, 64))
    assert _lib.load().pope_last_error() == b""


def insertion_csr(ei, n):
    """Rows by source; targets in order of first appearance of (u, v); one slot per distinct pair: the DiGraph's G[u]."""
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    _, first = np.unique(ei[0] * n + ei[1], return_index=True)
    first.sort()
    u, v = ei[0][first], ei[1][first]
    return np.concatenate([[0], np.cumsum(np.bincount(u, minlength=n))]).astype(np.int64), v[np.argsort(u, kind="stable")]


def replay_source(rp, col, rpi, coli, n, s, lanes=64):
    """One source of NetworkX 3.4.2's _single_source_shortest_path_basic + _accumulate_basic, restated as the kernel runs it:
    (sigma, delta, dist, reached).  delta[s] is computed and, as in NetworkX, not part of any score."""
    dist = np.full(n, -1, dtype=np.int64)
    sigma, delta = np.zeros(n), np.zeros(n)
    q = np.empty(n, dtype=np.int64)
    q[0] = s
    head, tail = 0, 1
    dist[s] = 0
    sigma[s] = 1.0
    while head < tail:
        v = q[head]
        head += 1
        for lo in range(rp[v], rp[v + 1], lanes):
            w = col[lo:min(lo + lanes, rp[v + 1])]
            new = w[dist[w] < 0]
            q[tail:tail + len(new)] = new
            tail += len(new)
            dist[new] = dist[v] + 1
            hit = w[dist[w] == dist[v] + 1]
            sigma[hit] = sigma[hit] + sigma[v]
    for i in range(tail - 1, -1, -1):
        w = q[i]
        coeff = (1 + delta[w]) / sigma[w]
        for lo in range(rpi[w], rpi[w + 1], lanes):
            p = coli[lo:min(lo + lanes, rpi[w + 1])]
            p = p[dist[p] == dist[w] - 1]
            delta[p] = delta[p] + sigma[p] * coeff                # a rounded product, then a rounded sum
    return sigma, delta, dist, tail


def replay(ei, n, lanes=64, normalized=True):
    """nx.betweenness_centrality(to_networkx(data)) restated: sources in node order, bc[w] the left-to-right sum of delta_s[w]."""
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    rp, col = insertion_csr(ei, n)
    rpi, coli = insertion_csr(ei[::-1], n)                        # predecessors: any order, de-duplicated
    bc = np.zeros(n)
    for s in range(n):
        _, delta, _, _ = replay_source(rp, col, rpi, coli, n, s, lanes)
        delta[s] = 0.0                                            # if w != s: betweenness[w] += delta[w]
        bc = bc + delta
    return bc * (1 / ((n - 1) * (n - 2))) if normalized and n > 2 else bc


def lattice(rows, cols, seed=0):
    """rows x cols grid, both directions of every edge, the edge list shuffled: many mathematically tied nodes."""
    idx = np.arange(rows * cols).reshape(rows, cols)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    ei = np.stack([np.concatenate([a, b]), np.concatenate([b, a])])
    return ei[:, np.random.RandomState(seed).permutation(ei.shape[1])].astype(np.int64), rows * cols


def networkx_scores(ei, n):
    import networkx as nx
    want = nx.betweenness_centrality(digraph(np.asarray(ei).reshape(2, -1), n))
    return np.array([want[v] for v in range(n)], dtype=np.float64)


def _golden():
    g = np.load(os.path.join(GOLDEN, "anchors_centrality.npz"))
    return g, g["edge_index"].astype(np.int64), int(g["num_nodes"])


def _spec_graphs():
    from graphpope_amd import synth
    _, ei, n = _golden()
    yield "golden", ei, n
    yield ("multigraph",) + random_multigraph()
    yield ("lattice_12x12",) + lattice(12, 12)
    yield ("rmat9_directed",) + synth.rmat(9, edge_factor=4, seed=13, symmetric=False)


@pytest.mark.parametrize("name", [g[0] for g in _spec_graphs()])
def test_restatement_is_networkx_bit_for_bit(name):
    _, ei, n = next(g for g in _spec_graphs() if g[0] == name)
    got, want = replay(ei, n), networkx_scores(ei, n)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(replay(ei, n, lanes=5).view(np.uint64), want.view(np.uint64))      # the chunking changes no sum


def test_restatement_selects_the_reference_anchors():
    """The last 24 of the ascending stable sort are the anchors the reference itself picked (golden)."""
    g, ei, n = _golden()
    assert np.argsort(replay(ei, n), kind="stable")[-24:].tolist() == g["betweenness_centrality"].tolist()


def test_restatement_degenerate_graphs():
    for ei, n in [(np.zeros((2, 0)), 1), (np.zeros((2, 0)), 2), (np.array([[0, 1], [1, 0]]), 2), (np.zeros((2, 0)), 6),
                  (np.array([[0], [0]]), 1), (np.array([[0, 1, 2, 2, 5], [1, 2, 0, 1, 2]]), 9)]:
        assert np.array_equal(replay(ei, n).view(np.uint64), networkx_scores(ei, n).view(np.uint64))


def _call(lib, ptrs, n=8, es=4, et=4, first=0, ns=4, scratch_bytes=1 << 20):
    r, c, rt, ct, bc, s = ptrs
    null = ctypes.c_void_p(0)
    return lib.pope_betweenness_batch(r, c, es, rt, ct, et, n, first, ns, bc, null, null, null, null, s, scratch_bytes, null)


def test_argument_validation_needs_no_gpu():
    """Null pointers, N <= 0, slot counts beyond int32 offsets, sources that are no nodes and a scratch that is too small are
    refused before any HIP call, with the function's name behind pope_last_error()."""
    from graphpope_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = [p] * 6
    for k in range(6):                                    # each required pointer in turn
        args = list(ok)
        args[k] = null
        assert _call(lib, args) == _lib.ERR_INVALID, k
        assert b"pope_betweenness_batch" in lib.pope_last_error() and b"null pointer" in lib.pope_last_error()
    for bad in (dict(n=0), dict(n=-1), dict(n=1 << 31), dict(es=-1), dict(et=-1), dict(first=-1), dict(ns=0), dict(ns=-3),
                dict(first=5, ns=4), dict(ns=9)):
        assert _call(lib, ok, **bad) == _lib.ERR_INVALID, bad
        assert b"pope_betweenness_batch" in lib.pope_last_error()
    assert _call(lib, ok, es=1 << 31) == _lib.ERR_INVALID and b"int32" in lib.pope_last_error()
    assert _call(lib, ok, et=(1 << 31) - 1) == _lib.ERR_INVALID and b"int32" in lib.pope_last_error()
    assert _call(lib, ok, n=(1 << 31) - 2, ns=1 << 20) == _lib.ERR_INVALID and b"too large" in lib.pope_last_error()
    # with no slots the column arrays are not needed; bc and the scratch still are
    assert _call(lib, [p, null, p, null, null, p], es=0, et=0) == _lib.ERR_INVALID
    assert _call(lib, [p, null, p, null, p, null], es=0, et=0) == _lib.ERR_INVALID
    # valid arguments, a scratch below the query's answer: POPE_ERR_WORKSPACE, still before any HIP call
    need = lib.pope_betweenness_scratch_bytes(8, 4)
    assert _call(lib, ok, scratch_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert b"pope_betweenness_batch" in lib.pope_last_error() and b"scratch" in lib.pope_last_error()


def test_scratch_query_needs_no_gpu():
    """The layout is arithmetic, so the query answers without a GPU: 36 bytes per (source, node) and the queue lengths, every
    part rounded up to 256 bytes; 0 for refused sizes."""
    from graphpope_amd import _lib
    lib = _lib.load()
    q = lib.pope_betweenness_scratch_bytes
    assert q(0, 1) == 0 and q(-5, 1) == 0 and q(10, 0) == 0 and q(10, -1) == 0 and q(1 << 31, 1) == 0
    assert q(10, 11) == 0                                                   # more sources than nodes
    assert q((1 << 31) - 2, 1 << 20) == 0                                   # beyond 2^40 (source, node) pairs

    def up(x):
        return (x + 255) // 256 * 256
    for n, b in ((1, 1), (8, 4), (89250, 1), (89250, 8192), (19717, 19717)):
        assert q(n, b) == up(n * b * 32) + up(n * b * 4) + up(b * 4), (n, b)
    assert lib.pope_last_error() == b""
