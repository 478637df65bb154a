"""Eigenvector-centrality anchors (utils.py:44-48 nx.eigenvector_centrality_numpy), the parts that need no GPU: the NumPy / SciPy
restatement of the device's power iteration, NetworkX's own ARPACK call without NetworkX 3's connectivity check, the
restatement-against-ARPACK differences the GPU tolerances are derived from, and the C ABI's argument checks.

Agreement with ARPACK is to a measured tolerance, never bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg

from conftest import GOLDEN, ROOT

TOL = 1e-13                       # engine.eigenvector_centrality's default stop rule: ||M^T x - lambda x|| <= TOL * lambda

# max |restatement - arpack_scores| per graph, as measured on the CPU (NumPy 2.2.6, SciPy 1.15.3) and asserted below with
# room for another BLAS / ARPACK build: the bound of the CPU test is 4 x the figure seen, and the GPU tests' bound is
# GPU_FACTOR x that (the device differs from the restatement in summation order only, within a row and within a reduction).
SEEN = {
    "golden": 8.7e-15,
    "star": 2.3e-14,
    "powerlaw800": 2.5e-14,
    "rmat9_directed": 8.2e-15,
    "pubmed": 2.1e-13,
    "flickr": 3.7e-14,
    "row_paths": 2.8e-14,
    "batched_rows": 3.6e-14,
}
CPU_BOUND = {k: 4.0 * v for k, v in SEEN.items()}
GPU_FACTOR = 10.0                 # the issue's: ten times the restatement-versus-ARPACK difference measured on the CPU
GPU_BOUND = {k: GPU_FACTOR * v for k, v in SEEN.items()}
TOP_K = {"golden": 24, "powerlaw800": 64, "rmat9_directed": 32, "pubmed": 256, "flickr": 256}
ITERATIONS = {"golden": 24, "star": 42, "powerlaw800": 47, "rmat9_directed": 21, "pubmed": 94, "flickr": 63, "row_paths": 36, "batched_rows": 73}


def adjacency(ei, n):
    """M: float64 SciPy CSR of the DiGraph to_networkx builds: one entry per distinct (u, v) pair, self-loops kept."""
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    key = np.unique(ei[0] * n + ei[1])
    return sp.csr_matrix((np.ones(len(key)), (key // n, key % n)), shape=(n, n))


def restate(ei, n, tol=TOL, max_iter=10_000):
    """The device's iteration in NumPy: (scores, iterations, lambda).  Start 1 / sqrt(N); ax = M^T x; lambda = x . ax;
    r = ||ax - lambda x||; stop if r <= tol * lambda; else x <- (ax + x) / ||ax + x||.  Scores = x / (sign(sum) * ||x||)."""
    at = adjacency(ei, n).T.tocsr()
    x = np.full(n, 1.0 / np.sqrt(n), dtype=np.float64)
    for it in range(1, max_iter + 1):
        ax = at @ x
        lam = float(x @ ax)
        r = float(np.linalg.norm(ax - lam * x))
        if r <= tol * lam:
            return x / (np.sign(x.sum()) * np.linalg.norm(x)), it, lam
        y = ax + x
        x = y / np.linalg.norm(y)
    raise RuntimeError(f"restatement: no convergence within {max_iter} iterations")


def arpack_scores(ei, n):
    """nx.eigenvector_centrality_numpy's own computation (NetworkX 3.4.2, max_iter=50, tol=0) without its connectivity check:
    what the reference's pinned NetworkX 2 returned on any graph."""
    m = adjacency(ei, n)
    _, vec = scipy.sparse.linalg.eigs(m.T, k=1, which="LR", maxiter=50, tol=0)
    largest = vec.flatten().real
    return largest / (np.sign(largest.sum()) * np.linalg.norm(largest))


def residual(ei, n, scores):
    """(||M^T x - lambda x||_2, lambda) of a score vector, lambda = x . M^T x / x . x."""
    at = adjacency(ei, n).T.tocsr()
    ax = at @ scores
    lam = float(scores @ ax) / float(scores @ scores)
    return float(np.linalg.norm(ax - lam * scores)), lam


def last_k(scores, k):
    return np.argsort(scores, kind="stable")[-k:].tolist()


def digraph(ei, n):
    import networkx as nx
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(np.asarray(ei[0]).tolist(), np.asarray(ei[1]).tolist()))
    return g


def star(leaves=8):
    """K_{1, leaves}, both directions: centre 0.  Bipartite: an unshifted power iteration alternates for ever."""
    a, b = np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1, dtype=np.int64)
    return np.stack([np.concatenate([a, b]), np.concatenate([b, a])]), leaves + 1


def _kernel_constant(name):
    """A `constexpr int` of csrc/eigenvector.hip: the graphs below are built around the kernel's own split lengths."""
    src = open(os.path.join(ROOT, "graphpope_amd", "csrc", "eigenvector.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


WAVE_ROW = _kernel_constant("EIG_WAVE_ROW")          # rows of at least this many CSR entries go to a whole wave
ROW_UNROLL = _kernel_constant("EIG_ROW_UNROLL")      # entries a thread loads together on its own row
WAVE_UNROLL = _kernel_constant("EIG_WAVE_UNROLL")    # 64-entry strides a wave loads together on a long row


def row_paths(seed=4):
    """N = 300 (two blocks of 256 rows, the second partly filled), edge list shuffled.  In-rows as the by-target CSR holds them,
    repeated entries included: node 0: 203 entries (sources 1 .. 200 and 298, source 64 three times: the repeats straddle the
    first 64-entry stride of the wave's loop; 203 is no multiple of 64), nodes 1, 2, 3: WAVE_ROW - 1, WAVE_ROW and WAVE_ROW + 1
    entries, node 5: a short row with one edge three times and a self-loop, node 299: no entry at all (it only points away).
    A two-way ring over 0 .. 298 keeps everything else in one strong component; 1 500 random edges among the other nodes give
    the spectrum a gap (40-odd iterations instead of 250)."""
    rs = np.random.RandomState(seed)
    src, dst = [], []

    def add(u, v):
        src.append(int(u))
        dst.append(int(v))

    ring = 299
    for i in range(ring):
        add(i, (i + 1) % ring)
        add((i + 1) % ring, i)
    for u, v in zip(rs.randint(0, ring, 1500), rs.randint(0, ring, 1500)):
        if v not in (0, 1, 2, 3, 5):
            add(u, v)
    for u in range(2, 201):                         # node 0: the ring gives 1 and 298; 2 .. 200 added, 64 twice more
        add(u, 0)
    add(64, 0)
    add(64, 0)
    for v, want in ((1, WAVE_ROW - 1), (2, WAVE_ROW), (3, WAVE_ROW + 1)):
        for u in range(100, 100 + want - 2):        # on top of the ring's two neighbours
            add(u, v)
    add(5, 5)                                       # self-loop
    for _ in range(3):
        add(250, 5)                                 # one edge three times
    add(299, 7)                                     # node 299 has an empty in-row
    add(299, 150)
    ei = np.array([src, dst], dtype=np.int64)
    ei = ei[:, rs.permutation(ei.shape[1])]
    n = 300
    rows = np.bincount(ei[1], minlength=n)
    assert rows[0] == 203 and list(rows[1:4]) == [WAVE_ROW - 1, WAVE_ROW, WAVE_ROW + 1] and rows[299] == 0 and rows[5] == 6
    return ei, n


def row_positions(ei, n, node):
    """The in-row of `node` as the canonical by-target CSR holds it: its sources ascending, repeats kept."""
    return np.sort(ei[0][ei[1] == node])


def batched_rows(seed=9):
    """N = 1 200, edge list shuffled: the batched loops of both row paths, with repeated edges at their seams.
    Node 0's in-row has 1 000 entries (sources 1 .. 992, four of them three times).  A lane takes entries l, l + 64, ... and
    loads WAVE_UNROLL = 8 strides (512 entries) together while 448 more lie ahead of it, so every lane runs one batch over
    entries 0 .. 511, lanes 0 .. 39 a second one over 512 + 64 u + l, and lanes 40 .. 63 finish in the one-stride tail loop;
    1 000 is neither a multiple of 512 nor of 64.  The repeats sit at entries 100-102 (inside one stride of a batch), 127-129
    (across two strides of a batch), 511-513 (across two batches) and 550-552 (lanes 38, 39: second batch; lane 40: tail).
    Node 1's in-row has 20 entries on the thread path, loaded ROW_UNROLL = 8 at a time, with a repeat at entries 7-9 (across
    two of its batches).  7 000 random edges among the other nodes give the spectrum a gap."""
    assert (WAVE_ROW, ROW_UNROLL, WAVE_UNROLL) == (64, 8, 8)       # the entry numbers above are worked out for these
    rs = np.random.RandomState(seed)
    n = 1200
    u, v = rs.randint(1, n, 7000), rs.randint(2, n, 7000)          # nothing random points at node 0 or 1
    src, dst = list(u), list(v)
    for s_ in range(1, 993):
        src.append(s_), dst.append(0)
    for s_ in (101, 126, 508, 545):                                # entry of source s = s - 1 + 2 x (repeated sources below s)
        src.extend([s_, s_]), dst.extend([0, 0])
    for s_ in range(2, 20):
        src.append(s_), dst.append(1)
    src.extend([9, 9]), dst.extend([1, 1])
    for t in range(2, n, 3):                                       # node 0 and node 1 feed the rest
        src.extend([0, 1]), dst.extend([t, t])
    ei = np.array([src, dst], dtype=np.int64)
    ei = ei[:, rs.permutation(ei.shape[1])]
    row0, row1 = row_positions(ei, n, 0), row_positions(ei, n, 1)
    assert len(row0) == 1000 and len(row0) % (64 * WAVE_UNROLL) and len(row0) % 64 and len(row0) >= 64 * WAVE_UNROLL + 64
    for first in (100, 127, 511, 550):
        assert row0[first] == row0[first + 1] == row0[first + 2] and row0[first - 1] != row0[first] != row0[first + 3]
    assert len(row1) == 20 < WAVE_ROW and row1[7] == row1[8] == row1[9] and row1[6] != row1[7] != row1[10]
    return ei, n


_cache = {}


def graph(name):
    """(edge_index int64 [2, E], N) of the graphs the tolerances are measured on; built once."""
    if name not in _cache:
        from graphpope_amd import synth
        if name == "golden":
            g = np.load(os.path.join(GOLDEN, "anchors_centrality.npz"))
            _cache[name] = g["edge_index"].astype(np.int64), int(g["num_nodes"])
        elif name == "star":
            _cache[name] = star(8)
        elif name == "powerlaw800":
            _cache[name] = synth.powerlaw_graph(800, 4000, seed=3, alpha=0.9, shift=0.8), 800
        elif name == "rmat9_directed":
            g = np.load(os.path.join(GOLDEN, "geodesic_rmat9_directed.npz"))
            _cache[name] = g["edge_index"].astype(np.int64), int(g["num_nodes"])
        elif name == "row_paths":
            _cache[name] = row_paths()
        elif name == "batched_rows":
            _cache[name] = batched_rows()
        elif name == "pubmed":
            _cache[name] = synth.pubmed_like()
        elif name == "flickr":
            _cache[name] = synth.flickr_like()
        else:
            raise KeyError(name)
    return _cache[name]


def reference(name):
    """arpack_scores of a named graph, computed once and shared (read-only)."""
    key = ("arpack", name)
    if key not in _cache:
        ei, n = graph(name)
        s = arpack_scores(ei, n)
        s.setflags(write=False)
        _cache[key] = s
    return _cache[key]


def restated(name):
    key = ("restate", name)
    if key not in _cache:
        ei, n = graph(name)
        s, its, lam = restate(ei, n)
        s.setflags(write=False)
        _cache[key] = (s, its, lam)
    return _cache[key]


def test_arpack_scores_is_networkx_on_a_strongly_connected_graph():
    """The same ARPACK call as NetworkX's.  ARPACK draws its start vector at random, so two calls of
    nx.eigenvector_centrality_numpy itself differ in the last bits (2.2e-16 seen on this graph, whose largest score is 0.31);
    the two functions are held to 5e-15, some twenty times that scatter, and to the same anchors in the same order."""
    import networkx as nx
    ei, n = graph("golden")
    g = digraph(ei, n)
    assert nx.is_strongly_connected(g)
    want = nx.eigenvector_centrality_numpy(g)
    want = np.array([want[v] for v in range(n)])
    again = nx.eigenvector_centrality_numpy(g)
    print(f"networkx against itself: {np.abs(want - np.array([again[v] for v in range(n)])).max():.3g}, "
          f"arpack_scores against networkx: {np.abs(reference('golden') - want).max():.3g}")
    assert np.abs(reference("golden") - want).max() <= 5e-15
    assert last_k(reference("golden"), 24) == last_k(want, 24)
    anchors = np.load(os.path.join(GOLDEN, "anchors_centrality.npz"))["eigenvector_centrality"].tolist()
    assert last_k(reference("golden"), 24) == anchors


@pytest.mark.parametrize("name", list(SEEN))
def test_restatement_against_arpack(name):
    """Where the tolerances come from: max |restatement - ARPACK| per graph, printed and held to 4 x the recorded figure; the
    iteration counts; the residual of the restatement's vector; the same last-K anchors in the same order."""
    ei, n = graph(name)
    got, its, lam = restated(name)
    want = reference(name)
    diff = float(np.abs(got - want).max())
    r, lam_host = residual(ei, n, got)
    print(f"{name}: N = {n}, iterations = {its}, lambda = {lam:.6g}, max |restatement - arpack| = {diff:.3g}, residual / lambda = {r / lam:.3g}")
    assert diff <= CPU_BOUND[name]
    assert abs(its - ITERATIONS[name]) <= 2             # another BLAS may cross the 1e-13 line an iteration earlier or later
    assert r <= 1e-12 * lam_host
    if name in TOP_K:
        k = TOP_K[name]
        assert last_k(got, k) == last_k(want, k)
        top = np.sort(want)[-(k + 1):]
        assert np.diff(top).min() >= 1.5e-7             # the gaps the exact comparison of the anchor lists rests on


def test_star_scores_are_exact():
    """K_{1,8}: lambda = sqrt(8), centre 1 / sqrt(2), leaves 1 / 4; fewer than 100 iterations although the graph is bipartite."""
    got, its, lam = restated("star")
    assert its < 100 and abs(lam - np.sqrt(8.0)) <= 1e-13
    assert abs(got[0] - 1.0 / np.sqrt(2.0)) <= 1e-13 and np.abs(got[1:] - 0.25).max() <= 1e-13


def test_disconnected_graphs_are_refused_by_networkx_3():
    """What the GPU path replaces: NetworkX 3 raises on the graphs the project trains on; ARPACK itself answers."""
    import networkx as nx
    for name in ("rmat9_directed", "powerlaw800"):
        ei, n = graph(name)
        with pytest.raises(nx.AmbiguousSolution):
            nx.eigenvector_centrality_numpy(digraph(ei, n))
        assert np.isfinite(reference(name)).all()


def test_argument_validation_needs_no_gpu():
    """Null pointers, N <= 0, iterations <= 0, tol <= 0 (and NaN) and a scratch that is too small are refused before any HIP
    call; the scratch query answers without a GPU."""
    from graphpope_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = lib.pope_eigenvector_scratch_bytes
    need = q(8)
    assert need >= 8 * 8 + 3 * 8

    def call(rowptr=p, src=p, x=p, scratch=p, control=p, n=8, scratch_bytes=need, iterations=1, tol=1e-13):
        return lib.pope_eigenvector_iterate(rowptr, src, n, x, scratch, scratch_bytes, iterations, tol, control, null)

    try:
        for name in ("rowptr", "src", "x", "scratch", "control"):
            assert call(**{name: null}) == _lib.ERR_INVALID, name
            assert b"pope_eigenvector_iterate" in lib.pope_last_error() and b"null pointer" in lib.pope_last_error()
        for n in (0, -1, (1 << 31) - 1, 1 << 31):
            assert call(n=n, scratch_bytes=1 << 40) == _lib.ERR_INVALID, n
            assert b"pope_eigenvector_iterate" in lib.pope_last_error()
        for tol in (0.0, -1e-13, float("nan")):
            assert call(tol=tol) == _lib.ERR_INVALID, tol
            assert b"tol" in lib.pope_last_error()
        assert call(iterations=0) == _lib.ERR_INVALID and call(iterations=-3) == _lib.ERR_INVALID
        assert call(scratch_bytes=need - 1) == _lib.ERR_WORKSPACE and call(scratch_bytes=0) == _lib.ERR_WORKSPACE
        assert b"pope_eigenvector_iterate" in lib.pope_last_error() and b"scratch" in lib.pope_last_error()
    finally:
        q(8)                        # a successful call clears the per-thread error string: the next test starts clean
    assert lib.pope_last_error() == b""

    assert q(0) == 0 and q(-5) == 0 and q((1 << 31) - 1) == 0 and q(1 << 40) == 0
    assert q(1) > 0
    assert q(89250) >= 89250 * 8 + 3 * 349 * 8                 # ax and three rows of per-block partials (349 blocks of 256 rows)
    assert q(1 << 22) >= (1 << 22) * 8 + 3 * 1024 * 8 and q(1 << 22) > q(89250)
