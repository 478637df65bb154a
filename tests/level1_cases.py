"""Graphs for the level-1 tests (tests/test_level1_hits_cpu.py, tests/test_level1_apply_gpu.py): the smallest shapes at which recording
the edges into anchors in the CSR pass and applying them in a small launch can go wrong.  Each case is (name, edge_index int64 [2, E]
sorted by source, num_nodes, anchors)."""
import numpy as np


def _sorted(src, dst):
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = np.lexsort((dst, src))
    return np.stack([src[order], dst[order]])


def random_graph(n, e, seed):
    """A directed multigraph with self-loops: e edges drawn uniformly, sorted by source."""
    rng = np.random.RandomState(seed)
    return _sorted(rng.randint(0, n, e), rng.randint(0, n, e))


def path(n):
    return np.stack([np.arange(n - 1, dtype=np.int64), np.arange(1, n, dtype=np.int64)])


def star(leaves):
    """Centre 0 -> every leaf (a row of `leaves` slots: four chunks of 256 at 1 000), every leaf -> centre."""
    ids = np.arange(1, leaves + 1, dtype=np.int64)
    return _sorted(np.concatenate([np.zeros(leaves, dtype=np.int64), ids]), np.concatenate([ids, np.zeros(leaves, dtype=np.int64)]))


def cases():
    out = []
    out.append(("path201_ends_and_middle", path(201), 201, [0, 100, 200]))          # depth 200: far beyond any depth hint
    g = random_graph(300, 2400, 1)
    out.append(("repeated_anchor_k5", g, 300, [17, 17, 3, 17, 250]))
    out.append(("k1", g, 300, [123]))
    out.append(("k256", g, 300, list(np.random.RandomState(2).choice(300, 256))))
    out.append(("k257_level_launch", g, 300, list(np.random.RandomState(3).choice(300, 257))))
    # 0: an anchor nobody points at; 1: an anchor with a self-loop; 2 <-> 3: two anchors pointing at each other; 4, 5, 6 feed them
    out.append(("no_in_edge_self_loop_mutual", _sorted([0, 1, 2, 3, 4, 5, 6, 6], [4, 1, 3, 2, 1, 2, 0, 5]), 7, [0, 1, 2, 3]))
    # no anchor has an in-edge: the BFS ends at level 1 with max_hop = 0
    out.append(("no_anchor_has_an_in_edge", _sorted([0, 1, 2, 3, 3], [2, 2, 3, 4, 5]), 6, [0, 1]))
    out.append(("star1000_spanning_row", star(1000), 1001, [0, 1, 2, 255, 256, 257, 500, 999, 1000]))
    e_odd = random_graph(200, 1501, 4)
    out.append(("e_odd", e_odd, 200, [0, 199, 57, 57]))
    out.append(("e0", np.zeros((2, 0), dtype=np.int64), 5, [0, 4]))
    out.append(("e1_into_anchor", np.array([[2], [3]], dtype=np.int64), 5, [3, 0]))
    out.append(("e1_out_of_anchor", np.array([[3], [2]], dtype=np.int64), 5, [3, 0]))
    out.append(("n33_partial_word", random_graph(33, 200, 5), 33, [32, 0, 31]))
    out.append(("n4097_partial_word", random_graph(4097, 30000, 6), 4097, [4096, 4095, 0, 2048, 4064]))
    return out


def equal_size_pair():
    """Two graphs of equal (N, E, K) with different edges and anchors: alternated on one workspace, a stale hit list or count shows."""
    return (("alt_a", random_graph(500, 4000, 7), 500, list(np.random.RandomState(8).choice(500, 40))),
            ("alt_b", random_graph(500, 4000, 9), 500, list(np.random.RandomState(10).choice(500, 40))))


def hit_slots(edge_index, anchors):
    """The CSR slots level 1 can use: the edges v -> u whose target u is an anchor (what k_prepare's CSR role records)."""
    return np.flatnonzero(np.isin(edge_index[1], np.asarray(anchors, dtype=np.int64)))


def level1_from_hits(edge_index, num_nodes, anchors):
    """bool [N, K]: (v, j) gains anchor j at level 1 -- an edge v -> anchors[j] exists and v is not anchors[j] itself (hop 0 stays 0)."""
    anchors = np.asarray(anchors, dtype=np.int64)
    got = np.zeros((num_nodes, anchors.size), dtype=bool)
    slots = hit_slots(edge_index, anchors)
    v, u = edge_index[0][slots], edge_index[1][slots]
    for j, a in enumerate(anchors):                       # front0[u] holds bit j for EVERY j with anchors[j] == u: repeats for free
        got[v[u == a], j] = True
    got[anchors, np.arange(anchors.size)] = False         # ... & ~seen[v]: the seeds
    return got
