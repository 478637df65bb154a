"""sampling_method='clustering_coefficient' (utils.py:56-60 nx.clustering) on the GPU: the device's exact integers give
NetworkX's float64 scores bit for bit, hence the reference's anchors."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_clustering_cpu import digraph, m_matrix, networkx_formula, random_multigraph, restate_counts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


class Data:
    pass


def _scores(ei, n, dev):
    from graphpope_amd import engine
    return engine.clustering_coefficient(torch.as_tensor(np.asarray(ei, dtype=np.int64).reshape(2, -1), device=dev), n)


def _networkx(ei, n, nodes=None):
    import networkx as nx
    want = nx.clustering(digraph(ei, n), nodes=None if nodes is None else [int(v) for v in nodes])
    return np.array([want[v] for v in (range(n) if nodes is None else [int(v) for v in nodes])], dtype=np.float64)


def _graphs():
    from graphpope_amd import synth
    g = np.load(os.path.join(GOLDEN, "anchors_centrality.npz"))
    yield "golden", g["edge_index"].astype(np.int64), int(g["num_nodes"])
    for sym in (True, False):
        ei, n = synth.rmat(9, edge_factor=4, seed=13, symmetric=sym)
        yield f"rmat9_{'sym' if sym else 'directed'}", ei, n
    yield ("multigraph",) + random_multigraph()
    yield "no_edges", np.zeros((2, 0), dtype=np.int64), 6
    yield "one_node", np.zeros((2, 0), dtype=np.int64), 1
    yield "one_node_self_loop", np.array([[0], [0]]), 1
    yield "reciprocal_pair", np.array([[0, 1], [1, 0]]), 2
    yield "isolated_nodes", np.array([[0, 1, 2, 2, 5], [1, 2, 0, 1, 2]]), 9           # nodes 3, 4, 6, 7, 8 isolated
    yield "triangle_with_loops", np.array([[0, 1, 2, 0, 1, 1], [1, 2, 0, 0, 0, 1]]), 4


@pytest.mark.parametrize("name", [g[0] for g in _graphs()])
def test_scores_are_networkx_bit_for_bit(name, dev):
    _, ei, n = next(g for g in _graphs() if g[0] == name)
    got = _scores(ei, n, dev)
    assert got.dtype == np.float64 and got.shape == (n,)
    assert np.array_equal(got.view(np.uint64), _networkx(ei, n).view(np.uint64))


def test_pubmed_shaped_bit_for_bit(dev):
    from graphpope_amd import synth
    ei, n = synth.pubmed_like()
    assert np.array_equal(_scores(ei, n, dev), _networkx(ei, n))


def test_reference_selection_comes_from_the_gpu(dev, monkeypatch):
    """With nx.clustering unusable the selection still equals the reference's own (golden); Graphpope over those anchors
    gives the same bits as a call whose scores come from nx.clustering."""
    import networkx as nx
    from graphpope_amd import engine, utils as gp
    g = np.load(os.path.join(GOLDEN, "anchors_centrality.npz"))
    ei, n = g["edge_index"].astype(np.int64), int(g["num_nodes"])
    want_scores = _networkx(ei, n)

    def refuse(*a, **k):
        raise AssertionError("nx.clustering called")

    d = Data()
    d.edge_index, d.num_nodes = torch.as_tensor(ei), n
    d.x = torch.as_tensor(np.random.RandomState(3).rand(n, 12).astype(np.float32))
    with monkeypatch.context() as m:
        m.setattr(nx, "clustering", refuse)
        assert gp.sample_anchor_nodes(d, 24, "clustering_coefficient") == g["clustering_coefficient"].tolist()
        gp.clear_cache()
        try:
            out = gp.Graphpope(d, "flickr", "geodesic", "clustering_coefficient", 24, None, 2).clone()
        finally:
            gp.clear_cache()
        anchors = list(d.anchor_nodes)
    assert anchors == g["clustering_coefficient"].tolist() and out.shape == (n, 12 + 24)
    with monkeypatch.context() as m:
        m.setattr(engine, "clustering_coefficient", lambda e, nn: want_scores.copy())
        try:
            want = gp.Graphpope(d, "flickr", "geodesic", "clustering_coefficient", 24, None, 2).clone()
        finally:
            gp.clear_cache()
    assert list(d.anchor_nodes) == anchors
    assert np.array_equal(out.numpy().view(np.uint32), want.numpy().view(np.uint32))


def test_flickr_shaped_full_size(dev):
    """All 89 250 (T, dt, db) against the SciPy restatement, the scores and the top-256 selection, and nx.clustering itself on
    500 sampled nodes that include the 10 of highest degree."""
    from graphpope_amd import engine, synth
    ei, n = synth.flickr_like()
    t, dt, db = engine.clustering_counts(torch.as_tensor(ei, device=dev), n)
    wt, wdt, wdb = restate_counts(m_matrix(ei, n))
    assert np.array_equal(dt, wdt) and np.array_equal(db, wdb) and np.array_equal(t, wt)
    want = networkx_formula(wt, wdt, wdb)
    got = engine.clustering_coefficient(torch.as_tensor(ei, device=dev), n)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.argsort(got, kind="stable")[-256:].tolist() == np.argsort(want, kind="stable")[-256:].tolist()
    top = np.argsort(wdt, kind="stable")[-10:]
    sample = np.unique(np.concatenate([top, np.random.RandomState(11).choice(n, 490, replace=False)]))
    assert len(sample) >= 495
    assert np.array_equal(got[sample].view(np.uint64), _networkx(ei, n, nodes=sample).view(np.uint64))


@pytest.mark.parametrize("reciprocal", [True, False])
def test_long_oriented_rows(reciprocal, dev):
    """Complete digraph K_n (every pair both ways, M = 2) and transitive tournament (one way, M = 1), n = 2 100: oriented rows
    of up to n - 1 = 2 099 entries, more than the 1 024 the triangle kernel stages at a time, so rows run in three chunks."""
    from graphpope_amd import engine
    n = 2100
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    keep = i != j if reciprocal else i < j
    ei = np.stack([i[keep], j[keep]]).astype(np.int64)
    ei = ei[:, np.random.RandomState(0).permutation(ei.shape[1])]
    eid = torch.as_tensor(ei, device=dev)
    t, dt, db = engine.clustering_counts(eid, n)
    w = 2 if reciprocal else 1
    assert (dt == w * (n - 1)).all() and (db == (n - 1 if reciprocal else 0)).all()
    assert (t == w ** 3 * (n - 1) * (n - 2)).all()
    score = engine.clustering_coefficient(eid, n)
    assert (score == (1.0 if reciprocal else 0.5)).all()


def test_rmat22(dev):
    """configs[4]'s graph: dt and db of every node against NumPy, T against the SciPy restatement on 200 random nodes and the
    3 of highest degree; every T even; a second call gives the same integers."""
    from graphpope_amd import engine, synth
    ei, n = synth.rmat(22, edge_factor=8, seed=1)
    eid = torch.as_tensor(ei, device=dev)
    t, dt, db = engine.clustering_counts(eid, n)
    src, dst = ei[0], ei[1]
    keep = src != dst
    key = np.unique(src[keep] * n + dst[keep])
    s, d = key // n, key % n
    recip = np.isin(d * n + s, key, assume_unique=True)
    assert np.array_equal(dt, np.bincount(s, minlength=n) + np.bincount(d, minlength=n))
    assert np.array_equal(db, np.bincount(s[recip], minlength=n))
    assert (t % 2 == 0).all() and t.min() >= 0
    rows = np.unique(np.concatenate([np.argsort(dt, kind="stable")[-3:], np.random.RandomState(2).choice(n, 200, replace=False)]))
    m = m_matrix(ei, n)
    wt, wdt, wdb = restate_counts(m, rows, chunk=16)
    assert np.array_equal(t[rows], wt) and np.array_equal(dt[rows], wdt) and np.array_equal(db[rows], wdb)
    assert (t[rows] > 0).sum() >= 40                                       # 43 of these rows lie on a triangle
    t2, dt2, db2 = engine.clustering_counts(eid, n)
    assert np.array_equal(t, t2) and np.array_equal(dt, dt2) and np.array_equal(db, db2)


def _oriented(ei, n):
    """Host restatement of the oriented graph: per node, the neighbours after it in the order (distinct degree, id), as the
    device encodes them (k << 1 | [M_ik == 2]), ascending."""
    m = m_matrix(ei, n)
    deg = np.diff(m.indptr)
    rows = []
    for i in range(n):
        ks, ws = m.indices[m.indptr[i]:m.indptr[i + 1]], m.data[m.indptr[i]:m.indptr[i + 1]]
        after = (deg[ks] > deg[i]) | ((deg[ks] == deg[i]) & (ks > i))
        rows.append(np.sort((ks[after].astype(np.int64) << 1) | (ws[after] == 2)))
    return rows


@pytest.mark.parametrize("name", ["tournament", "rmat9_directed", "multigraph", "isolated_nodes", "golden"])
def test_oriented_rows_stay_inside_their_buffers(name, dev):
    """Directed inputs: the oriented row offsets start at 0 and end at the number of unordered pairs (<= E, the room the
    scratch layout gives the oriented rows), the rows are the host's oriented neighbour lists, and nothing is written past
    the scratch the query asked for (a poisoned guard tail stays intact).  Reads rowptr and rows at their offsets in the
    scratch layout of csrc/clustering.hip (cl_layout): code [2E + 1] B | scan [2E + 1] u64 | degree [N] | rowptr [N + 1] |
    rows unsorted [E] | rows sorted [E], every part aligned to 256 bytes."""
    from graphpope_amd import _lib, engine
    if name == "tournament":
        n = 300
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        ei = np.stack([i[i < j], j[i < j]]).astype(np.int64)
    else:
        _, ei, n = next(g for g in _graphs() if g[0] == name)
    ei = np.asarray(ei, dtype=np.int64)
    e = ei.shape[1]
    lib = _lib.load()
    eid = torch.as_tensor(ei, device=dev)
    s, t = engine.build_csr_canonical(eid, n), engine.build_csr_canonical(eid.flip(0).contiguous(), n)
    need = lib.pope_clustering_scratch_bytes(n, e)
    guard = 1 << 20
    scratch = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.empty((3, n), dtype=torch.int64, device=dev)
    _lib.check(lib.pope_clustering_counts(_lib.ptr(s.rowptr), _lib.ptr(s.col), _lib.ptr(s.erow), _lib.ptr(t.rowptr), _lib.ptr(t.col),
                                          _lib.ptr(t.erow), n, e, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]),
                                          _lib.ptr(scratch), need, engine._stream()))
    torch.cuda.synchronize()
    assert bool((scratch[need:] == 0xA5).all())

    def up(x):
        return (x + 255) // 256 * 256
    o_rp = up(2 * e + 1) + up((2 * e + 1) * 8) + up(n * 4)
    o_nbr = o_rp + up((n + 1) * 4) + up(max(e, 1) * 4)
    rp = scratch[o_rp:o_rp + 4 * (n + 1)].view(torch.int32).cpu().numpy()
    want = _oriented(ei, n)
    pairs = sum(len(r) for r in want)
    assert rp[0] == 0 and rp[n] == pairs <= e
    assert np.array_equal(np.diff(rp), [len(r) for r in want])
    nbr = scratch[o_nbr:o_nbr + 4 * pairs].view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    for i in range(n):
        assert np.array_equal(nbr[rp[i]:rp[i + 1]], want[i]), i
    assert np.array_equal(out[0].cpu().numpy(), restate_counts(m_matrix(ei, n))[0])
