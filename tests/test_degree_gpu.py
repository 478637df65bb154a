"""sampling_method='degree_centrality' (utils.py:38-42 nx.degree_centrality, the command line's default) on the GPU: exact integer
degrees, NetworkX's float64 scores bit for bit, and the K largest keys degree << 32 | node selected on the device -- the list
sample_anchor_nodes returned from the host before, for every input.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_degree_cpu import SELECT_N, cli_graph, digraph, host_anchors, host_degrees, key_sets, select_ks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


class Data:
    pass


def _golden():
    g = np.load(os.path.join(GOLDEN, "anchors_centrality.npz"))
    return g, g["edge_index"].astype(np.int64), int(g["num_nodes"])


def _repeated(times):
    return np.stack([np.full(times, 3), np.full(times, 1)]), 5


def _graphs():
    from graphpope_amd import synth
    _, ei, n = _golden()
    yield "golden", ei, n
    yield ("cli",) + cli_graph()
    ei, n = synth.rmat(9, edge_factor=4, seed=13, symmetric=True)
    yield "rmat9_sym", ei, n
    ei, n = synth.rmat(9, edge_factor=4, seed=13, symmetric=False)
    yield "rmat9_directed_shuffled", ei[:, np.random.RandomState(4).permutation(ei.shape[1])], n
    yield "first_target_equals_previous_slot", np.array([[0, 1], [5, 5]]), 6
    for times in (65, 257, 1000):
        yield (f"one_edge_{times}_times",) + _repeated(times)
    hub = np.stack([np.full(1000, 700), np.concatenate([np.arange(0, 700), np.arange(701, 1001)])])
    yield "hub_beside_empty_rows", hub[:, np.random.RandomState(1).permutation(1000)], 1200
    yield "only_a_self_loop", np.array([[0, 4, 2], [1, 4, 0]]), 6
    yield "no_edges", np.zeros((2, 0), dtype=np.int64), 6
    yield "one_node", np.zeros((2, 0), dtype=np.int64), 1
    yield "one_node_self_loop", np.array([[0, 0], [0, 0]]), 1


@pytest.mark.parametrize("name", [g[0] for g in _graphs()])
def test_degrees_and_scores_are_exact(name, dev):
    import networkx as nx
    from graphpope_amd import engine
    _, ei, n = next(g for g in _graphs() if g[0] == name)
    ei = np.asarray(ei, dtype=np.int64)
    eid = torch.as_tensor(ei, device=dev)
    deg = engine.degree_counts(eid, n)
    assert deg.is_cuda and deg.dtype == torch.int64 and deg.shape == (n,)
    assert np.array_equal(deg.cpu().numpy(), host_degrees(ei, n))
    got = engine.degree_centrality(eid, n)
    dc = nx.degree_centrality(digraph(ei, n))
    want = np.array([dc[v] for v in range(n)], dtype=np.float64)
    assert got.dtype == np.float64 and got.shape == (n,)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if name == "only_a_self_loop":
        assert deg.cpu().numpy()[4] == 2


def test_padded_tail_is_never_read(dev):
    """E no multiple of 64: the padded tail of col / erow holds 0x7F bytes (node 2 139 062 143, far outside the graph) when
    pope_degree_counts runs; the slots end at rowptr[N]."""
    from graphpope_amd import _lib, engine
    ei, n = cli_graph()
    e = ei.shape[1]
    assert e % 64 != 0
    csr = engine.build_csr_canonical(torch.as_tensor(ei, device=dev), n)
    assert csr.col.numel() > e and csr.erow.numel() > e
    csr.col[e:] = 0x7F7F7F7F
    csr.erow[e:] = 0x7F7F7F7F
    deg = torch.full((n,), -1, dtype=torch.int64, device=dev)
    keys = torch.full((n,), -1, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().pope_degree_counts(_lib.ptr(csr.rowptr), _lib.ptr(csr.col), _lib.ptr(csr.erow), n, _lib.ptr(deg), _lib.ptr(keys),
                                              engine._stream()))
    want = host_degrees(ei, n)
    assert np.array_equal(deg.cpu().numpy(), want)
    assert np.array_equal(keys.cpu().numpy(), (want << 32) | np.arange(n))


# ------------------------------------------------------------------------------------------------ anchors
def test_reference_selection_comes_from_the_gpu(dev, monkeypatch):
    """The golden list, with edge_index on the host and on the device, through engine.degree_anchors (recorded)."""
    from graphpope_amd import engine, utils as gp
    g, ei, n = _golden()
    calls = []
    real = engine.degree_anchors

    def recording(edge_index, num_nodes, k):
        calls.append((edge_index.device.type, int(num_nodes), k))
        return real(edge_index, num_nodes, k)

    monkeypatch.setattr(engine, "degree_anchors", recording)
    want = g["degree_centrality"].tolist()
    for t in (torch.as_tensor(ei), torch.as_tensor(ei, device=dev)):
        d = Data()
        d.edge_index, d.num_nodes = t, n
        got = gp.sample_anchor_nodes(d, len(want), "degree_centrality")
        assert isinstance(got, list) and all(type(v) is int for v in got) and got == want
    assert calls == [("cuda", n, len(want))] * 2


def test_every_k_gives_the_host_list(dev):
    from graphpope_amd import engine, synth
    _, ei, n = _golden()
    eid = torch.as_tensor(ei, device=dev)
    for k in (1, 12, n - 1, n, n + 3, 0):
        assert engine.degree_anchors(eid, n, k) == host_anchors(ei, n, k), k
    cap = engine.topk_max_k()
    ei, n = synth.rmat(13, edge_factor=4, seed=5)
    assert n > cap + 1
    eid = torch.as_tensor(ei, device=dev)
    for k in (cap, cap + 1):
        got = engine.degree_anchors(eid, n, k)
        assert len(got) == k and got == host_anchors(ei, n, k), k


def test_no_edges_gives_the_last_k_ids(dev):
    from graphpope_amd import engine
    eid = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    assert engine.degree_anchors(eid, 300, 7) == list(range(293, 300))
    assert engine.degree_anchors(eid, 300, 0) == list(range(300))
    assert engine.degree_anchors(eid, 1, 1) == [0]


def test_star_leaves_tie_and_the_hub_comes_last(dev):
    from graphpope_amd import engine
    n, hub = 200, 57
    leaves = np.array([v for v in range(n) if v != hub])
    ei = np.stack([np.full(n - 1, hub), leaves])
    got = engine.degree_anchors(torch.as_tensor(ei, device=dev), n, 10)
    assert got == leaves[-9:].tolist() + [hub] and got == host_anchors(ei, n, 10)


# ------------------------------------------------------------------------------------------------ the select itself
def _select(keys_dev, n, k, scratch, out):
    from graphpope_amd import _lib, engine
    _lib.check(_lib.load().pope_topk_u64(_lib.ptr(keys_dev), n, k, _lib.ptr(out), _lib.ptr(scratch), scratch.numel(), engine._stream()))
    return out[:k].cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("n", SELECT_N)
def test_topk_is_the_sorted_tail(n, dev):
    """pope_topk_u64 against np.sort(keys)[-K:] on every key set; each call runs twice, the scratch filled with 0xFF bytes in
    between (whatever the scratch holds on entry, the call initialises what it reads), with identical output.  A guard behind
    the scratch and behind the K result slots stays intact."""
    from graphpope_amd import _lib, engine
    lib = _lib.load()
    cap = engine.topk_max_k()
    guard = 4096
    for k in select_ks(n, cap):
        need = lib.pope_topk_scratch_bytes(n, k)
        assert need > 0
        scratch = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=dev)
        out = torch.full((k + 8,), -1, dtype=torch.int64, device=dev)
        for name, keys in key_sets(n, k):
            want = np.sort(keys)[-k:]
            keys_dev = torch.as_tensor(keys.view(np.int64), device=dev)
            first = _select(keys_dev, n, k, scratch[:need], out)
            assert np.array_equal(first, want), (name, k)
            scratch[:need] = 0xFF
            second = _select(keys_dev, n, k, scratch[:need], out)
            assert np.array_equal(second, first), (name, k)
        assert bool((scratch[need:] == 0xA5).all()) and bool((out[k:] == -1).all()), k


# ------------------------------------------------------------------------------------------------ Flickr-shaped
@pytest.fixture(scope="module")
def flickr():
    from graphpope_amd import synth
    ei, n = synth.flickr_like()
    return ei, n, host_anchors(ei, n, 256)


def test_flickr_shaped_twice_in_a_row(flickr, dev):
    from graphpope_amd import engine
    ei, n, want = flickr
    eid = torch.as_tensor(ei, device=dev)
    assert engine.degree_anchors(eid, n, 256) == want
    assert engine.degree_anchors(eid, n, 256) == want


def test_graphpope_call_with_the_default_sampling_method(dev):
    from graphpope_amd import utils as gp
    g, ei, n = _golden()
    d = Data()
    d.edge_index, d.num_nodes = torch.as_tensor(ei), n
    d.x = torch.as_tensor(np.random.RandomState(3).rand(n, 12).astype(np.float32))
    want = g["degree_centrality"].tolist()
    gp.clear_cache()
    try:
        out = gp.Graphpope(d, "flickr", "geodesic", "degree_centrality", len(want))
        assert list(d.anchor_nodes) == want and out.shape == (n, 12 + len(want))
    finally:
        gp.clear_cache()
