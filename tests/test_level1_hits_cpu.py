"""Level 1 of the multi-source BFS restated from the edges into anchors alone (no GPU): the slots k_prepare's CSR role records are
the edges whose target is an anchor, and the rows k_bfs_level1_apply builds from them are exactly the pairs with hop count 1.
Checked against the C oracle on the graphs of tests/level1_cases.py; on the benchmark's graph and anchors the number of such slots is
pinned -- 2 424 of 899 756, the figure the design rests on."""
import numpy as np
import pytest

import level1_cases as lc


@pytest.mark.parametrize("case", lc.cases() + list(lc.equal_size_pair()), ids=lambda c: c[0])
def test_hits_give_exactly_the_pairs_at_hop_one(case, oracle):
    _, ei, n, anchors = case
    hops = oracle.geodesic_hops(ei, n, anchors)
    assert np.array_equal(lc.level1_from_hits(ei, n, anchors), hops == 1)
    assert np.array_equal(hops[np.asarray(anchors), np.arange(len(anchors))], np.zeros(len(anchors), dtype=np.int32))


def test_benchmark_graph_has_2424_hit_slots(oracle):
    from graphpope_amd import synth
    ei, n = synth.flickr_like(seed=1)
    anchors = synth.seeded_anchors(n, 256, 42)
    slots = lc.hit_slots(ei, anchors)
    assert ei.shape[1] == 899756 and slots.size == 2424
    assert np.unique(slots >> 8).size == 1760                       # spread over half of the 3 515 chunks of 256 slots
    hops = oracle.geodesic_hops(ei, n, anchors)
    assert np.array_equal(lc.level1_from_hits(ei, n, anchors), hops == 1)
    assert int(hops.max()) == 9
