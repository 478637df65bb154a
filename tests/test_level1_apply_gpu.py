"""Level 1 from the CSR pass (POPE_KNOB_LEVEL1_APPLY, the default): k_prepare's CSR role records the edges into anchors and
k_bfs_level1_apply applies them in place of the first launch of the level kernel.  Every case compares engine.hop_matrix of
engine.geodesic_run bit for bit with the C oracle on the same input AND with the same call under the knob off (the level launch);
the profile's launch record says which of the two kernels ran level 1."""
import numpy as np
import pytest
import torch

import level1_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


@pytest.fixture()
def lib():
    from graphpope_amd import _lib
    lib = _lib.load()
    lib.pope_debug_set(_lib.KNOB_LEVEL1_APPLY, 1)
    yield lib
    lib.pope_debug_set(_lib.KNOB_LEVEL1_APPLY, 1)
    lib.pope_profile_levels(0)


def _hops(lib, ei_dev, n, anchors, apply, reuse=False):
    """(hop matrix, max_hop, level-1 launches that were the apply kernel) of one geodesic_run under the knob."""
    from graphpope_amd import _lib, engine
    lib.pope_debug_set(_lib.KNOB_LEVEL1_APPLY, apply)
    lib.pope_profile_levels(2)
    try:
        _, hp = engine.geodesic_run(None, ei_dev, n, anchors, want_out=False, reuse_workspace=reuse)
        hops = engine.hop_matrix(hp).cpu().numpy()
        return hops, hp.max_hop, lib.pope_profile_level1_applies()
    finally:
        lib.pope_profile_levels(0)
        lib.pope_debug_set(_lib.KNOB_LEVEL1_APPLY, 1)


def _check(lib, dev, oracle, ei, n, anchors, expect_apply, reuse=False):
    ei_dev = torch.as_tensor(ei, device=dev)
    want = oracle.geodesic_hops(ei, n, anchors)
    got, max_hop, applies = _hops(lib, ei_dev, n, anchors, 1, reuse)
    off, max_hop_off, applies_off = _hops(lib, ei_dev, n, anchors, 0, reuse)
    assert applies == (1 if expect_apply else 0) and applies_off == 0
    assert np.array_equal(got, want) and np.array_equal(off, want)
    assert max_hop == max_hop_off == int(want.max())
    return want


@pytest.mark.parametrize("case", lc.cases(), ids=lambda c: c[0])
def test_same_bits_as_the_oracle_and_as_the_level_launch(case, lib, dev, oracle):
    """The shapes of tests/level1_cases.py: a path far deeper than the depth hint (the general path takes over behind the apply launch),
    repeated anchors, K = 1 and 256, K = 257 (the separate launches: the level kernel runs level 1), an anchor without in-edge / with a
    self-loop / two pointing at each other, no anchor with an in-edge (max_hop = 0: launch 2 finds the BFS over), hits on a row that
    spans four chunks from several blocks, E odd (the one-edge CSR role), E = 0 and 1, N = 33 and 4 097 (a partial last bitmap word)."""
    name, ei, n, anchors = case
    expect_apply = len(anchors) <= 256 and ei.shape[1] > 0            # k_prepare runs for at most 256 anchors and E > 0
    want = _check(lib, dev, oracle, ei, n, anchors, expect_apply)
    if name == "no_anchor_has_an_in_edge":
        assert int(want.max()) == 0
    if name == "path201_ends_and_middle":
        assert int(want.max()) == 200


def test_node_id_out_of_range_fails_alike(lib, dev):
    """The last edge points at node N: the CSR role flags it, never indexes its bitmap with it, and the call fails with the same error
    under either knob value; the workspace stays usable."""
    from graphpope_amd import _lib, engine
    ei = lc.random_graph(100, 800, 11)
    ei[1, -1] = 100
    ei_dev = torch.as_tensor(ei, device=dev)
    messages = []
    for apply in (1, 0):
        lib.pope_debug_set(_lib.KNOB_LEVEL1_APPLY, apply)
        with pytest.raises(_lib.PopeError) as e:
            engine.geodesic_run(None, ei_dev, 100, [0, 99, 5], want_out=False, reuse_workspace=True)
        assert e.value.code == _lib.ERR_INDEX
        messages.append(str(e.value))
    assert messages[0] == messages[1]


def test_unsorted_edge_list_takes_the_fallback(lib, dev, oracle):
    """Not sorted by source: the CSR role raises its flag, the hit lists are ignored (the apply launch returns at once) and the BFS
    starts over from the level launch on the counting-sort CSR."""
    ei = lc.random_graph(400, 3000, 12)
    ei = np.ascontiguousarray(ei[:, np.random.RandomState(13).permutation(ei.shape[1])])
    _check(lib, dev, oracle, ei, 400, [7, 399, 7, 21], expect_apply=True)


def test_reused_workspace_poisoned_between_calls(lib, dev, oracle):
    """One workspace for every call: overwritten with 0xFF and with random bytes in between (nothing the apply launch reads may be
    left over: counts and lists are written by every wave of the CSR role, the buffers it ORs into are zeroed by k_prepare), then two
    graphs of equal (N, E, K) alternating, so a hit list or a count of the other graph would show."""
    from graphpope_amd import engine
    a, b = lc.equal_size_pair()
    for rnd in range(3):
        for ws in engine._WORKSPACE.values():
            if rnd == 1:
                ws.fill_(0xFF)
            elif rnd == 2:
                ws.copy_(torch.randint(0, 256, ws.shape, dtype=torch.uint8, device=ws.device))
        _check(lib, dev, oracle, a[1], a[2], a[3], True, reuse=True)
    assert len(engine._WORKSPACE) >= 1
    for _, ei, n, anchors in (b, a, b, a):
        _check(lib, dev, oracle, ei, n, anchors, True, reuse=True)


def test_benchmark_shape(lib, dev, oracle):
    """The Flickr-shaped graph with the benchmark's 256 anchors: the planes equal the level launch's bit for bit, max_hop = 9."""
    from graphpope_amd import _lib, engine, synth
    ei, n = synth.flickr_like(seed=1)
    anchors = synth.seeded_anchors(n, 256, 42)
    ei_dev = torch.as_tensor(ei, device=dev)
    lib.pope_debug_set(_lib.KNOB_LEVEL1_APPLY, 0)
    hp_off = engine.geodesic_run(None, ei_dev, n, anchors, want_out=False)[1]
    want = hp_off.valid().clone()
    lib.pope_debug_set(_lib.KNOB_LEVEL1_APPLY, 1)
    for _ in range(3):                                                 # the second call on runs under the depth hint
        hp = engine.geodesic_run(None, ei_dev, n, anchors, want_out=False, reuse_workspace=True)[1]
        assert hp.max_hop == 9 and hp_off.max_hop == 9
        assert torch.equal(hp.valid(), want)
    _check(lib, dev, oracle, ei, n, anchors, True, reuse=True)
