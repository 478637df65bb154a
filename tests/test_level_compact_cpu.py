"""How sparse the level launches of the benchmark's BFS are (no GPU): a numpy restatement of the level loop on the Flickr-shaped graph
with the benchmark's 256 anchors, counting for every launch the live slots of each 256-slot chunk -- a slot v -> u is live when the
frontier row of u is not all zero, which is when the level kernel gathers for it.  The figures are the table the compacted path of
k_bfs_level rests on (lesson 24): launches 8, 9 and 10 have at most 9 live slots in any chunk, launches 2 and 7
at most 128 in all but one.  Whoever changes the benchmark's graph or anchors learns here that the measurements no longer hold."""
import numpy as np
import pytest

import level_compact_cases as cc


@pytest.fixture(scope="module")
def bench_levels():
    from graphpope_amd import synth
    ei, n = synth.flickr_like(seed=1)
    anchors = synth.seeded_anchors(n, 256, 42)
    assert n == 89250 and ei.shape[1] == 899756
    levels, hops = cc.level_loop(ei, n, anchors)
    return ei, n, anchors, levels, hops


def test_restatement_is_the_oracles_bfs(bench_levels, oracle):
    ei, n, anchors, levels, hops = bench_levels
    assert np.array_equal(hops, oracle.geodesic_hops(ei, n, anchors))
    assert [l for l, _, _ in levels] == list(range(1, 11)) and int(hops.max()) == 9     # launch 10 finds nothing and proves the end


def test_live_slots_per_chunk_of_the_benchmark_bfs(bench_levels):
    _, _, _, levels, _ = bench_levels
    per = {l: c for l, c, _ in levels}
    gains = {l: g for l, _, g in levels}
    assert all(c.size == 3515 for c in per.values())
    busy = {l: int((c > 0).sum()) for l, c in per.items()}
    assert busy == {1: 1760, 2: 3515, 3: 3515, 4: 3515, 5: 3515, 6: 3515, 7: 3386, 8: 2538, 9: 65, 10: 1}
    # the sparse launches: maxima of live slots in a chunk
    assert [int(per[l].max()) for l in (1, 2, 7, 8, 9, 10)] == [6, 197, 123, 9, 2, 1]
    assert int((per[2] <= 128).sum()) == 3514                      # all but one chunk of launch 2 take the compacted path
    for l in (3, 4, 5):
        assert int((per[l] <= 128).sum()) == 0                     # the dense launches never do
    assert int((per[6] <= 128).sum()) == 2
    # median / 99th percentile over the busy chunks
    def med_p99(l):
        c = np.sort(per[l][per[l] > 0])
        return int(np.median(c)), int(c[int(np.ceil(0.99 * c.size)) - 1])
    assert med_p99(1) == (1, 3) and med_p99(2) == (41, 59) and med_p99(7) == (89, 110) and med_p99(8) == (2, 6)
    assert med_p99(9)[0] == 1 and int((per[9] == 2).sum()) == 1    # 65 busy chunks: 64 with one live slot, one with two
    for l in (3, 4, 5, 6):
        assert 213 <= med_p99(l)[0] <= 256
    # chunks that produce a new bit
    assert [int(gains[l].sum()) for l in (1, 2, 7, 8, 9, 10)] == [1760, 3515, 1939, 63, 1, 0]
    assert all(3249 <= int(gains[l].sum()) <= 3515 for l in (3, 4, 5, 6))


@pytest.mark.parametrize("case", cc.cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("k", [64, 256])
def test_cases_show_the_live_counts_they_are_named_for(case, k, oracle):
    """The graphs of the GPU test: the restatement agrees with the oracle on them, some chunk of some launch has exactly each live-slot
    count the case is built for, and every case has a chunk on the compacted path under the default threshold (1 .. 16 live slots)."""
    _, ei, n, hot, cold, want = case
    anchors = cc.anchors(k, hot, cold)
    levels, hops = cc.level_loop(ei, n, anchors)
    assert np.array_equal(hops, oracle.geodesic_hops(ei, n, anchors))
    counts = np.concatenate([c for l, c, _ in levels if l >= 2])       # launch 1 never takes the path
    for m in want:
        assert (counts == m).any()
    assert ((counts >= 1) & (counts <= 16)).any()
