"""Graphs and the numpy level loop for the tests of the level kernel's compacted path (tests/test_level_compact_cpu.py,
tests/test_level_compact_gpu.py).  A slot v -> u of the CSR is LIVE in the launch of a level when the frontier row of u is not all
zero; a 256-slot chunk with at most POPE_KNOB_LEVEL_COMPACT live slots (16; at most 64) takes the compacted path from launch 2 on.  Each case is
(name, edge_index int64 [2, E] sorted by source, num_nodes, hot, cold, want): the anchors of a K-anchor call are `anchors(K, hot, cold)`
-- the nodes that start the search at scattered bit positions, nodes without any edge at the others -- and `want` lists live-slot
counts that some chunk of some launch must show exactly (checked on the CPU, so a case keeps testing what its name says)."""
import numpy as np

import level1_cases as lc

CHUNK = 256


def level_loop(edge_index, num_nodes, anchors):
    """[(level, live slots per chunk int64 [nchunks], chunks with a slot that brings a new bit bool [nchunks])] for every launch up to
    and including the one that finds nothing, and the hop matrix int32 [N, K] (-1: unreachable) the loop arrives at."""
    src, dst = edge_index[0], edge_index[1]
    assert np.all(np.diff(src) >= 0)                               # slot p is edge p: the list is sorted by source
    k = len(anchors)
    w = (k + 63) // 64
    nchunks = (src.size + CHUNK - 1) // CHUNK
    front = np.zeros((num_nodes, w), dtype=np.uint64)
    for j, a in enumerate(anchors):
        front[a, j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    seen = front.copy()
    hops = np.full((num_nodes, k), -1, dtype=np.int32)
    hops[np.asarray(anchors), np.arange(k)] = 0
    out = []
    level = 1
    while True:
        live = np.flatnonzero(front.any(axis=1)[dst])             # the slots whose neighbour's live bit is set
        per_chunk = np.bincount(live >> 8, minlength=nchunks)
        cand = front[dst[live]] & ~seen[src[live]]                # seen holds front already: the kernel's seen[v] | front[v]
        gains = np.zeros(nchunks, dtype=bool)
        gains[np.unique(live[cand.any(axis=1)] >> 8)] = True
        new = np.zeros_like(front)
        if live.size:
            rows = src[live]
            starts = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
            new[rows[starts]] = np.bitwise_or.reduceat(cand, starts, axis=0)
        out.append((level, per_chunk, gains))
        if not new.any():
            return out, hops
        bits = np.unpackbits(new.view(np.uint8), axis=1, bitorder="little")[:, :k].astype(bool)
        hops[bits] = level
        seen |= new
        front = new
        level += 1


def anchors(k, hot, cold):
    """k anchors: `hot` nodes at every third position (so every one is drawn more than once and their bits lie in every word), `cold`
    nodes -- isolated: no edge in or out -- at the others."""
    return [int(hot[(j // 3) % len(hot)]) if j % 3 == 0 else int(cold[j % len(cold)]) for j in range(k)]


def star(m, leaves=256, extra=()):
    """Centre 0 -> leaves 1 .. `leaves` (its row fills whole chunks from slot 0), the leaves listed in m (or the first m) -> node A,
    one node -> the centre, two isolated nodes.  With A as the anchor the launch of level 1 finds the leaves' rows (one slot each) and
    the launch of level 2 finds len(m) live slots in the centre's row, in the chunks the leaves' slots fall into."""
    picked = np.arange(1, m + 1) if np.isscalar(m) else np.asarray(m)
    a = leaves + 1
    src = np.concatenate([np.zeros(leaves, dtype=np.int64), picked, [a + 1], [e[0] for e in extra]]).astype(np.int64)
    dst = np.concatenate([np.arange(1, leaves + 1), np.full(picked.size, a), [0], [e[1] for e in extra]]).astype(np.int64)
    return lc._sorted(src, dst), a + 4, [a], [a + 2, a + 3]


def degrees_one_and_two(seed, n=640, pool=24, hot=8):
    """Rows of out-degree 1 and 2 in random order (so their slots straddle lanes and chunk boundaries at every offset), every edge into
    a pool of `pool` nodes of which the first `hot` point at the anchor: hot / pool of the slots are live in launch 2."""
    rng = np.random.RandomState(seed)
    deg = rng.randint(1, 3, n)
    src = np.repeat(np.arange(n), deg)
    dst = n + rng.randint(0, pool, src.size)
    a = n + pool + 2
    src, dst = np.concatenate([src, n + np.arange(hot)]), np.concatenate([dst, np.full(hot, a)])
    return lc._sorted(src, dst), a + 1, [a], [n + pool, n + pool + 1]


def with_isolated(ei, n, hot):
    return ei, n + 2, hot, [n, n + 1]


def cases():
    out = []
    # 16 / 17: the last count on the compacted path and the first beyond it under the default; 64 / 65: under the largest threshold
    for m in (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129):
        out.append(("star_%d_live_slots" % m,) + star(m) + ([m],))
    # a hub row over three chunks (600 slots): its pieces are OR-ed in with atomics, as head or tail row of each chunk
    out.append(("hub_live_in_first_piece",) + star([3, 4, 200], 600) + ([3],))
    out.append(("hub_live_in_last_piece",) + star([520, 599, 600], 600) + ([3],))
    out.append(("hub_live_in_all_pieces",) + star([1, 256, 257, 300, 512, 513, 600], 600) + ([2, 3],))
    # leaves 1 .. 522 live: two chunks of the hub row on the general path and ten slots of its last piece compacted OR into one row
    out.append(("hub_general_and_compacted_pieces",) + star(np.arange(1, 523), 600) + ([256, 10],))
    out.append(("degrees_1_and_2_a",) + degrees_one_and_two(21, pool=64, hot=3) + ([],))          # about 12 live slots per chunk in launch 2
    out.append(("degrees_1_and_2_b",) + degrees_one_and_two(22, n=515, pool=9, hot=2) + ([],))
    # a short last chunk, and less than one chunk
    for e in (513, 511, 100):
        out.append(("random_e%d" % e,) + with_isolated(lc.random_graph(200, e, 30 + e % 7), 200, [5, 77, 199]) + ([],))
    # repeated targets inside a chunk and a self-loop on a frontier node and on the anchor (a multigraph on 12 nodes)
    multi = lc._sorted([0, 0, 0, 1, 1, 2, 3, 3, 3, 3, 4, 5, 5, 6, 7, 7, 8, 9], [3, 3, 3, 3, 1, 1, 9, 9, 3, 9, 0, 4, 4, 5, 6, 6, 7, 9])
    out.append(("repeated_targets_self_loops",) + with_isolated(multi, 10, [9]) + ([3],))
    # every level sparse, deeper than the 12 levels enqueued up front
    out.append(("path_40",) + with_isolated(lc.path(40), 40, [39, 20]) + ([1, 2],))
    return out
