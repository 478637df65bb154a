"""The compacted path of the level kernel (POPE_KNOB_LEVEL_COMPACT, default 16, at most 64): a 256-slot chunk with at most that many
live slots compacts them across the wave, one (v, u) pair per lane, and loads front[u], seen[v] and front[v] in one round trip.  Every
case compares the hop matrix with the C oracle and the raw planes, bit for bit, with the same call under the knob at 0 (every chunk on
the general path) and at 64 (the most the path takes) -- through engine.geodesic_run (level 1 from the hit lists, the level kernel
from level 2) AND engine.bfs (level 1 a launch of the level kernel, which keeps to the general path), with 64, 128 and 256 anchors (k_bfs_level<1 | 2 | 4, 1, 0>).  The graphs: tests/level_compact_cases.py."""
import numpy as np
import pytest
import torch

import level_compact_cases as cc

pytestmark = pytest.mark.gpu

KS = (64, 128, 256)
DEFAULT = 16


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


@pytest.fixture()
def lib():
    from graphpope_amd import _lib
    lib = _lib.load()
    lib.pope_debug_set(_lib.KNOB_LEVEL_COMPACT, DEFAULT)
    yield lib
    lib.pope_debug_set(_lib.KNOB_LEVEL_COMPACT, DEFAULT)


def _planes(lib, threshold, run):
    """(valid planes, hop matrix, max_hop) of run() under the knob; copies: a reused workspace is overwritten by the next call."""
    from graphpope_amd import _lib, engine
    lib.pope_debug_set(_lib.KNOB_LEVEL_COMPACT, threshold)
    try:
        hp = run()
        return hp.valid().clone(), engine.hop_matrix(hp).cpu().numpy(), hp.max_hop
    finally:
        lib.pope_debug_set(_lib.KNOB_LEVEL_COMPACT, DEFAULT)


def _check(lib, dev, oracle, ei, n, anchors, reuse=False):
    from graphpope_amd import engine
    ei_dev = torch.as_tensor(ei, device=dev)
    csr = engine.build_csr(ei_dev, n)
    want = oracle.geodesic_hops(ei, n, anchors)
    for run in (lambda: engine.geodesic_run(None, ei_dev, n, anchors, want_out=False, reuse_workspace=reuse)[1], lambda: engine.bfs(csr, anchors)):
        planes, hops, max_hop = _planes(lib, DEFAULT, run)
        assert np.array_equal(hops, want) and max_hop == int(want.max())
        for threshold in (0, 64):
            planes_t, hops_t, max_hop_t = _planes(lib, threshold, run)
            assert np.array_equal(hops_t, want) and max_hop_t == max_hop
            assert torch.equal(planes_t, planes)


@pytest.mark.parametrize("case", cc.cases(), ids=lambda c: c[0])
def test_same_bits_as_the_oracle_and_as_the_general_path(case, lib, dev, oracle):
    """Chunks with exactly 1, 2, 15, 16, 17, 63, 64, 65, 127, 128 and 129 live slots; a hub row over three chunks with live slots in its
    first piece, its last piece, all pieces, and two pieces on the general path with the third compacted (all OR into one row); rows
    of one and two slots across lanes and chunk boundaries; E % 256 of 1 and 255 and E < 256; repeated targets, self-loops, anchors drawn many times
    and anchors without an edge; a path deeper than the levels enqueued up front."""
    _, ei, n, hot, cold, _ = case
    for k in KS:
        _check(lib, dev, oracle, ei, n, cc.anchors(k, hot, cold))


def test_reused_workspace_poisoned_between_calls(lib, dev, oracle):
    """One workspace for every call, overwritten with 0xFF in between: front[v] of a row whose live bit is clear is loaded by the
    compacted path whatever it holds, and must be masked away."""
    from graphpope_amd import engine
    picked = [c for c in cc.cases() if c[0] in ("star_16_live_slots", "hub_live_in_all_pieces", "degrees_1_and_2_a", "path_40")]
    assert len(picked) == 4
    for rnd in range(2):
        for _, ei, n, hot, cold, _ in picked:
            for ws in engine._WORKSPACE.values():
                ws.fill_(0xFF)
            _check(lib, dev, oracle, ei, n, cc.anchors(256, hot, cold), reuse=True)
            for ws in engine._WORKSPACE.values():
                ws.fill_(0xFF)
            _check(lib, dev, oracle, ei, n, cc.anchors(64, hot, cold), reuse=True)
    assert len(engine._WORKSPACE) >= 1


def test_repeated_calls_give_identical_planes(lib, dev):
    """The same call three times on one workspace: identical planes (the atomic pieces of spanning rows commute)."""
    from graphpope_amd import engine
    for name in ("hub_general_and_compacted_pieces", "degrees_1_and_2_a"):
        _, ei, n, hot, cold, _ = next(c for c in cc.cases() if c[0] == name)
        ei_dev = torch.as_tensor(ei, device=dev)
        anchors = cc.anchors(256, hot, cold)
        first = None
        for _ in range(3):
            hp = engine.geodesic_run(None, ei_dev, n, anchors, want_out=False, reuse_workspace=True)[1]
            planes = hp.valid().clone()
            assert first is None or torch.equal(planes, first)
            first = planes


def test_benchmark_shape(lib, dev, oracle):
    """The Flickr-shaped graph with the benchmark's 256 anchors: launches 8, 9 and 10 run wholly on the compacted path, 2 and 7 in
    part, at 64 almost wholly (tests/test_level_compact_cpu.py); the planes equal the general path's bit for bit, and the oracle's hops."""
    from graphpope_amd import synth
    ei, n = synth.flickr_like(seed=1)
    _check(lib, dev, oracle, ei, n, synth.seeded_anchors(n, 256, 42), reuse=True)
