"""sampling_method='eigenvector_centrality' (utils.py:44-48 nx.eigenvector_centrality_numpy) on the GPU: a shifted float64
power iteration with the loop resident on the device.  Scores are compared with NetworkX's own ARPACK call to a tolerance
derived from CPU measurements (test_eigenvector_cpu.SEEN x GPU_FACTOR), never bit for bit; anchor lists are compared exactly
on graphs whose neighbouring scores lie at least 1.5e-7 apart."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_eigenvector_cpu import (GPU_BOUND, ROW_UNROLL, TOP_K, WAVE_ROW, WAVE_UNROLL, digraph, graph, last_k, reference, residual,
                                  restated, row_positions)

pytestmark = pytest.mark.gpu

GRAPHS = ["golden", "star", "row_paths", "batched_rows", "rmat9_directed", "powerlaw800", "pubmed", "flickr"]


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


class Data:
    pass


_scores = {}


def scores(name, dev):
    """engine.eigenvector_centrality of a named graph, computed once and shared (read-only)."""
    if name not in _scores:
        from graphpope_amd import engine
        ei, n = graph(name)
        s = engine.eigenvector_centrality(torch.as_tensor(ei, device=dev), n)
        assert s.dtype == np.float64 and s.shape == (n,)
        s.setflags(write=False)
        _scores[name] = s
    return _scores[name]


def _compare(name, dev):
    got = scores(name, dev)
    d_ref = float(np.abs(got - reference(name)).max())
    d_res = float(np.abs(got - restated(name)[0]).max())
    print(f"{name}: max |gpu - arpack| = {d_ref:.3g}, max |gpu - restatement| = {d_res:.3g}, bound {GPU_BOUND[name]:.3g}")
    assert d_ref <= GPU_BOUND[name] and d_res <= GPU_BOUND[name]
    assert abs(np.linalg.norm(got) - 1.0) <= 4e-16 and got.sum() > 0
    return got


def test_golden_scores_and_reference_anchors(dev, monkeypatch):
    """The reference's own 24 anchors, in order, from the device: NetworkX's call is made unusable for the selection."""
    import networkx as nx
    from graphpope_amd import utils as gp
    g = np.load(os.path.join(GOLDEN, "anchors_centrality.npz"))
    want = g["eigenvector_centrality"].tolist()
    got = _compare("golden", dev)
    assert last_k(got, 24) == want

    def refuse(*a, **k):
        raise AssertionError("nx.eigenvector_centrality_numpy called")

    d = Data()
    d.edge_index, d.num_nodes = torch.as_tensor(g["edge_index"].astype(np.int64)), int(g["num_nodes"])
    with monkeypatch.context() as m:
        m.setattr(nx, "eigenvector_centrality_numpy", refuse)
        assert gp.sample_anchor_nodes(d, 24, "eigenvector_centrality") == want


def test_star_converges_although_bipartite(dev):
    """K_{1,8}, N = 9: centre 1 / sqrt(2), leaves 1 / 4; the unshifted iteration alternates between two vectors for ever."""
    from graphpope_amd import engine
    got = _compare("star", dev)
    assert abs(got[0] - 1.0 / np.sqrt(2.0)) <= 1e-13 and np.abs(got[1:] - 0.25).max() <= 1e-13
    ei, n = graph("star")
    again = engine.eigenvector_centrality(torch.as_tensor(ei, device=dev), n, max_iter=99)      # fewer than 100 iterations
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))


def test_every_row_path(dev):
    """One thread per row, one wave per row, the lengths either side of the split, a row that is no multiple of the wave,
    an empty row, a self-loop, repeated edges in a short and in a long row, two blocks, a shuffled edge list."""
    ei, n = graph("row_paths")
    rows = np.bincount(ei[1], minlength=n)
    assert rows.max() > WAVE_ROW and rows.max() % 64 and {WAVE_ROW - 1, WAVE_ROW, WAVE_ROW + 1} <= set(rows.tolist())
    assert rows.min() == 0 and n % 256 and n > 256 and (ei[0] == ei[1]).any()
    for u, v in ((64, 0), (250, 5)):                                     # an edge three times in a wave row and in a thread row
        assert int(((ei[0] == u) & (ei[1] == v)).sum()) == 3
    got = _compare("row_paths", dev)
    assert 0.0 <= got[299] < 1e-30                                       # nothing feeds it: only the shift keeps it, divided by 1 + lambda per iteration


def test_batched_loops_and_their_seams(dev):
    """A 1 000-entry row: every lane runs one eight-stride batch, lanes 0 .. 39 a second one, lanes 40 .. 63 the tail loop,
    with an edge three times inside a stride, across two strides of a batch, across two batches and across the second batch
    and the tail; a 20-entry thread row with an edge three times across two of its eight-entry batches.  A repeat counted
    twice, or one dropped, moves node 0's score by a whole x[j]: far outside the bound."""
    ei, n = graph("batched_rows")
    row0, row1 = row_positions(ei, n, 0), row_positions(ei, n, 1)
    batch = 64 * WAVE_UNROLL
    assert len(row0) >= batch + 64 and len(row0) % batch and len(row0) % 64
    second = sum(lane + batch + (batch - 64) < len(row0) for lane in range(64))   # lanes whose second batch fits: 0 .. 39
    assert 0 < second < 64
    for first in (100, 127, 511, 550):
        assert row0[first] == row0[first + 2]
    assert ROW_UNROLL < len(row1) < WAVE_ROW and row1[ROW_UNROLL - 1] == row1[ROW_UNROLL + 1]
    _compare("batched_rows", dev)


@pytest.mark.parametrize("name", ["rmat9_directed", "powerlaw800"])
def test_disconnected_graphs(name, dev):
    """270 strong components (directed) and 16 components (symmetric): NetworkX 3 refuses both, ARPACK itself answers, and
    the device returns its scores and its anchors."""
    import networkx as nx
    ei, n = graph(name)
    with pytest.raises(nx.AmbiguousSolution):
        nx.eigenvector_centrality_numpy(digraph(ei, n))
    got = _compare(name, dev)
    assert last_k(got, TOP_K[name]) == last_k(reference(name), TOP_K[name])


@pytest.mark.parametrize("name", ["pubmed", "flickr"])
def test_full_size_graphs(name, dev):
    """The PubMed- and the Flickr-shaped graph whole (1 254 and 1 159 components; a row of some 5 400 entries on the wave path):
    ARPACK's scores and its last 256 anchors in order."""
    got = _compare(name, dev)
    assert last_k(got, 256) == last_k(reference(name), 256)


def test_determinism_and_check_every(dev):
    """Two calls return the same bits; so do check_every = 1 and 8 (and 5: a group that ends mid-way), on a graph with wave
    rows and several blocks and on the smallest one."""
    from graphpope_amd import engine
    for name in ("row_paths", "batched_rows", "flickr", "star"):
        ei, n = graph(name)
        eid = torch.as_tensor(ei, device=dev)
        first = scores(name, dev)
        for every in (8, 1, 5) if name != "flickr" else (8, 1):
            again = engine.eigenvector_centrality(eid, n, check_every=every)
            assert np.array_equal(again.view(np.uint64), first.view(np.uint64)), (name, every)


@pytest.mark.parametrize("name", GRAPHS)
def test_residual_needs_no_reference(name, dev):
    """||M^T x - lambda x||_2 recomputed in NumPy from the returned scores is at most 1e-12 lambda: the device stops at 1e-13,
    and the host's other summation order moves the figure by far less than the remaining factor of ten."""
    ei, n = graph(name)
    r, lam = residual(ei, n, scores(name, dev))
    print(f"{name}: lambda = {lam:.6g}, residual / lambda = {r / lam:.3g}")
    assert abs(lam - restated(name)[2]) <= 1e-12 * lam
    assert r <= 1e-12 * lam


def test_iteration_count_and_control_block(dev):
    """The control block after convergence: done set, the restatement's iteration count give or take one (the summation order
    may cross the 1e-13 line an iteration earlier or later), lambda and r; the launches queued behind write nothing."""
    from graphpope_amd import _lib, engine
    lib = _lib.load()
    ei, n = graph("row_paths")
    t = engine.build_csr_canonical(torch.as_tensor(ei, device=dev).flip(0).contiguous(), n)
    x = torch.as_tensor(np.full(n, 1.0 / np.sqrt(n)), device=dev)
    control = torch.zeros(4, dtype=torch.int64, device=dev)
    need = lib.pope_eigenvector_scratch_bytes(n)
    guard = 4096
    scratch = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=dev)
    want_iterations = restated("row_paths")[1]
    _lib.check(lib.pope_eigenvector_iterate(_lib.ptr(t.rowptr), _lib.ptr(t.col), n, _lib.ptr(x), _lib.ptr(scratch), need,
                                            want_iterations + 1, 1e-13, _lib.ptr(control), engine._stream()))
    torch.cuda.synchronize()
    state = control.cpu().numpy()
    lam, r = state[1:3].view(np.float64)
    assert state[3] == 1 and abs(int(state[0]) - want_iterations) <= 1
    assert abs(lam - restated("row_paths")[2]) <= 1e-12 * lam and 0.0 <= r <= 1e-13 * lam
    assert bool((scratch[need:] == 0xA5).all())
    before = x.clone()
    _lib.check(lib.pope_eigenvector_iterate(_lib.ptr(t.rowptr), _lib.ptr(t.col), n, _lib.ptr(x), _lib.ptr(scratch), need,
                                            8, 1e-13, _lib.ptr(control), engine._stream()))
    torch.cuda.synchronize()
    assert torch.equal(x, before) and np.array_equal(control.cpu().numpy(), state)
    v = x.cpu().numpy()
    assert np.array_equal(v / (np.sign(v.sum()) * np.linalg.norm(v)), scores("row_paths", dev))


def test_no_convergence_raises_and_leaves_nothing_behind(dev):
    """A three-node directed path is acyclic (lambda = 0): RuntimeError after max_iter iterations, as engine.pagerank; an empty
    edge list raises too; the next call starts from a clean control block."""
    from graphpope_amd import engine
    path = torch.as_tensor(np.array([[0, 1], [1, 2]], dtype=np.int64), device=dev)
    with pytest.raises(RuntimeError, match="failed to converge within 64 iterations"):
        engine.eigenvector_centrality(path, 3, max_iter=64)
    with pytest.raises(RuntimeError, match="failed to converge within 5 iterations"):
        engine.eigenvector_centrality(path, 3, max_iter=5, check_every=8)
    with pytest.raises(RuntimeError, match="no edges"):
        engine.eigenvector_centrality(torch.zeros((2, 0), dtype=torch.int64, device=dev), 6)
    ei, n = graph("star")
    again = engine.eigenvector_centrality(torch.as_tensor(ei, device=dev), n)
    assert np.array_equal(again.view(np.uint64), scores("star", dev).view(np.uint64))
