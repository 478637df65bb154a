"""The K best anchors of the five score-ranked sampling methods, selected on the device (utils.py:29-30 and the same two lines of
every method: ascending stable sort of the float64 scores, last K): pope_topk_f64 against np.argsort(scores, kind="stable")[-K:]
element for element, engine.score_anchors, and each method through sample_anchor_nodes.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_anchor_select_cpu import SELECT_N, host_line, score_families, select_ks

pytestmark = pytest.mark.gpu

METHODS = ("closeness_centrality", "pagerank", "clustering_coefficient", "betweenness_centrality", "eigenvector_centrality")


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


class Data:
    pass


# ------------------------------------------------------------------------------------------------ the select itself
@pytest.mark.parametrize("n", SELECT_N)
def test_topk_f64_is_the_tail_of_the_stable_sort(n, dev):
    """Every score family and K; each call runs twice, the scratch filled with 0xFF bytes in between (whatever the scratch holds
    on entry, the call initialises what it reads), with identical output.  Guards behind the scratch and behind both outputs stay
    intact; scores_out is bitwise scores[nodes_out], and may be left out."""
    from graphpope_amd import _lib, engine
    lib = _lib.load()
    cap = engine.topk_max_k()
    assert SELECT_N[-1] == 1024 * 256 + 77                                # TOPK_GRID_CAP * TOPK_BLOCK + 77: two trips of the loop, ragged
    guard = 4096
    ks = select_ks(n, cap)
    assert ks and (n <= cap or cap in ks)
    families = list(score_families(n))
    for name, x in families:
        order = np.argsort(x, kind="stable")
        x_dev = torch.as_tensor(x, device=dev)
        for k in ks:
            need = lib.pope_topk_f64_scratch_bytes(n, k)
            assert need > 0
            scratch = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=dev)
            nodes = torch.full((k + 8,), -1, dtype=torch.int64, device=dev)
            vals = torch.full((k + 8,), -1, dtype=torch.int64, device=dev)      # float64 bit patterns
            want = order[-k:]

            def run(with_scores):
                _lib.check(lib.pope_topk_f64(_lib.ptr(x_dev), n, k, _lib.ptr(nodes), _lib.ptr(vals) if with_scores else None,
                                             _lib.ptr(scratch), need, engine._stream()))
                return nodes[:k].cpu().numpy()

            first = run(True)
            assert np.array_equal(first, want), (name, k)
            assert np.array_equal(vals[:k].cpu().numpy().view(np.uint64), x[want].view(np.uint64)), (name, k)
            scratch[:need] = 0xFF
            vals[:k] = -1
            second = run(k != ks[0])                                       # the smallest K: without scores_out
            assert np.array_equal(second, first), (name, k)
            if k == ks[0]:
                assert bool((vals == -1).all()), (name, k)
            else:
                assert np.array_equal(vals[:k].cpu().numpy().view(np.uint64), x[want].view(np.uint64)), (name, k)
            assert bool((scratch[need:] == 0xA5).all()) and bool((nodes[k:] == -1).all()) and bool((vals[k:] == -1).all()), (name, k)
            assert np.array_equal(want, host_line(x, k))


# ------------------------------------------------------------------------------------------------ engine.score_anchors
def test_score_anchors_host_array_and_device_tensor(dev):
    """A host array and a device tensor give the same list; k = 0, N, N + 3, the cap, cap + 1 and a negative k are Python's slice
    of the host sort."""
    from graphpope_amd import engine
    cap = engine.topk_max_k()
    n = cap + 904
    rs = np.random.RandomState(11)
    x = rs.choice(np.array([0.0, 0.0, 0.0, 1.0, 0.5, 1.0 / 3.0, 0.25]), n)      # clustering-like: mostly ties
    x[rs.permutation(n)[:300]] = rs.rand(300)
    x_dev = torch.as_tensor(x, device=dev)
    order = np.argsort(x, kind="stable")
    for k in (0, n, n + 3, cap, cap + 1, -5, 1, 24, np.int64(256)):
        want = order[-k:].tolist()
        from_host = engine.score_anchors(x, k)
        from_dev = engine.score_anchors(x_dev, k)
        assert isinstance(from_host, list) and all(type(v) is int for v in from_host[:50])
        assert from_host == want and from_dev == want, k
    assert len(engine.score_anchors(x, cap)) == cap and len(engine.score_anchors(x, cap + 1)) == cap + 1
    assert engine.score_anchors(np.zeros(0), 3) == [] and engine.score_anchors(np.array([2.5]), 1) == [0]


def test_score_anchors_runs_the_device_select_only_where_it_applies(dev, monkeypatch):
    from graphpope_amd import _lib, engine
    lib = _lib.load()
    cap = engine.topk_max_k()
    calls = []
    real = lib.pope_topk_f64

    def recording(scores, n, k, *rest):
        calls.append((int(n), int(k)))
        return real(scores, n, k, *rest)

    monkeypatch.setattr(lib, "pope_topk_f64", recording)
    x = np.random.RandomState(2).rand(cap + 10)
    n = len(x)
    for k in (1, 24, cap):
        engine.score_anchors(x, k)
    assert calls == [(n, 1), (n, 24), (n, cap)]
    for k in (0, n, cap + 1, n + 3, -5):
        engine.score_anchors(x, k)
    assert len(calls) == 3


# ------------------------------------------------------------------------------------------------ the five methods
def _golden():
    g = np.load(os.path.join(GOLDEN, "anchors_centrality.npz"))
    return g, g["edge_index"].astype(np.int64), int(g["num_nodes"])


def _star_with_pendant_paths():
    """A hub with 36 arms, paths of 6 and of 5 nodes alternately, both directions of every edge, node labels shuffled: N = 199.
    Nodes at the same depth of equally long arms tie in every score; every clustering coefficient is 0."""
    edges, nxt = [], 1
    for arm in range(36):
        prev = 0
        for _ in range(6 if arm % 2 == 0 else 5):
            edges += [(prev, nxt), (nxt, prev)]
            prev, nxt = nxt, nxt + 1
    n = nxt
    relabel = np.random.RandomState(5).permutation(n)
    ei = relabel[np.array(edges, dtype=np.int64).T]
    return ei[:, np.random.RandomState(6).permutation(ei.shape[1])], n


@pytest.mark.parametrize("method", METHODS)
def test_each_method_selects_on_the_device(method, dev, monkeypatch):
    """sample_anchor_nodes with edge_index on the host and on the device: the golden list on the golden graph, and on both graphs
    the host line over the very scores engine.<method> returns; engine.score_anchors and pope_topk_f64 are recorded."""
    from graphpope_amd import _lib, engine, utils as gp
    lib = _lib.load()
    anchors_calls, select_calls = [], []
    real_anchors, real_select = engine.score_anchors, lib.pope_topk_f64

    def recording_anchors(score, k):
        anchors_calls.append((type(score).__name__, len(score), k))
        return real_anchors(score, k)

    def recording_select(scores, n, k, *rest):
        select_calls.append((int(n), int(k)))
        return real_select(scores, n, k, *rest)

    monkeypatch.setattr(engine, "score_anchors", recording_anchors)
    monkeypatch.setattr(lib, "pope_topk_f64", recording_select)
    g, ei, n = _golden()
    star_ei, star_n = _star_with_pendant_paths()
    assert 190 <= star_n <= 210
    k = len(g[method])
    for name, e, nn, want in (("golden", ei, n, g[method].tolist()), ("star", star_ei, star_n, None)):
        score = getattr(engine, method)(torch.as_tensor(e, device=dev), nn)
        assert isinstance(score, np.ndarray) and score.dtype == np.float64 and score.shape == (nn,)
        line = np.argsort(score, kind="stable")[-k:].tolist()
        if name == "star" and method != "eigenvector_centrality":          # (the power iteration may tell automorphic nodes apart in the last bit)
            assert len(np.unique(score)) <= nn // 4                        # heavy ties
        del anchors_calls[:], select_calls[:]
        for t in (torch.as_tensor(e), torch.as_tensor(e, device=dev)):
            d = Data()
            d.edge_index, d.num_nodes = t, nn
            got = gp.sample_anchor_nodes(d, k, method)
            assert isinstance(got, list) and all(type(v) is int for v in got)
            assert got == line, (name, t.device.type)
            if want is not None:
                assert got == want, (name, t.device.type)
        assert anchors_calls == [("ndarray", nn, k)] * 2 and select_calls == [(nn, k)] * 2, name
