"""Shared by tests/test_node2vec_det_cpu.py and tests/test_node2vec_det_gpu.py: the contract of pope_n2v_accumulate_det
(include/graphpope_hip.h) restated as a NumPy loop, the "cancellation lists" whose sum shows the order it was taken in, and the case
the ordered-sum GPU test runs.  Not a test module."""
import numpy as np

N = 70
M = 3000
LONG, IN65, IN64, IN1 = 5, 11, 12, 13               # nodes with 1 500, 65, 64 and 1 entries
SPREAD = range(20, 60)                              # the other entries land here; 0-4, 6-10, 14-19 and 60-69 have none
SKIPPED = 10                                        # entries with id -1, and as many with id N


def accumulate_reference(ids, contrib, grad, order=None):
    """(grad after the call, touched): per node a float64 accumulator that takes the node's contrib rows in ascending entry order
    (or in ``order``, a sequence of entries, to show that another order gives another result), one rounding to float32 at the end.
    Entries outside [0, n) are skipped; nodes without entries keep their row bit for bit."""
    n, d = grad.shape
    acc = np.zeros((n, d), dtype=np.float64)
    seen = np.zeros(n, dtype=bool)
    for e in (range(len(ids)) if order is None else order):
        v = int(ids[e])
        if 0 <= v < n:
            acc[v] = acc[v] + contrib[e].astype(np.float64)
            seen[v] = True
    out = grad.copy()
    out[seen] = (grad[seen].astype(np.float64) + acc[seen]).astype(np.float32)
    return out, seen.astype(np.uint8)


def cancellation_lists(ids, n, d, rng):
    """contrib float32 [M, d] of N(0, 1) values in which two entries of every list (a node's entries, per column) are replaced by +b
    and -b, b = 2^80 k with an integer k in [1, 2^20).  In a float64 accumulator +b swallows what was added before it and whatever
    comes until -b arrives; only what follows the pair survives.  Which entries those are depends on the order: a sum taken in
    another order ends in other bits, which plain random values (all exact in float64 at these lengths) never show."""
    contrib = rng.standard_normal((len(ids), d)).astype(np.float32)
    for v in range(n):
        entries = np.nonzero(ids == v)[0]
        if len(entries) < 2:
            continue
        for col in range(d):
            first, second = rng.choice(entries, size=2, replace=False)
            b = np.float32(np.ldexp(float(rng.integers(1, 1 << 20)), 80))
            contrib[first, col], contrib[second, col] = b, -b
    return contrib


def ordered_sum_ids(rng):
    """int32 [M] in shuffled entry order: the list lengths the sum kernel treats differently (1 500: longer than a wave, than a block
    and than 1 024; 65; 64; 1; none), and ids -1 and N, which the call skips."""
    fixed = [LONG] * 1500 + [IN65] * 65 + [IN64] * 64 + [IN1] + [-1] * SKIPPED + [N] * SKIPPED
    rest = rng.choice(np.array(SPREAD), size=M - len(fixed))
    ids = np.concatenate([np.array(fixed), rest]).astype(np.int32)
    rng.shuffle(ids)
    count = np.bincount(ids[(ids >= 0) & (ids < N)], minlength=N)
    assert len(ids) == M and count[LONG] == 1500 and count[IN65] == 65 and count[IN64] == 64 and count[IN1] == 1
    assert (count[list(range(0, 5)) + list(range(60, 70))] == 0).all() and (ids == -1).sum() == SKIPPED and (ids == N).sum() == SKIPPED
    return ids


def ordered_sum_case(d, seed=0):
    """(ids [M], contrib [M, d], prior grad [N, d]) of the ordered-sum test at width d."""
    rng = np.random.default_rng(seed)
    ids = ordered_sum_ids(rng)
    contrib = cancellation_lists(ids, N, d, rng)
    grad = rng.standard_normal((N, d)).astype(np.float32)
    return ids, contrib, grad


SCAN_ROUND = 8192                                   # entries the one-block scan of the index takes per round (1024 threads x 8)
CARRY_N = 2 * SCAN_ROUND + 3                        # three rounds, the last with 3 entries
CARRY_HUB = SCAN_ROUND                              # the first node of round 1
CARRY_LISTS = {0: 60, SCAN_ROUND - 1: 64, CARRY_HUB: 70, 2 * SCAN_ROUND - 1: 65, 2 * SCAN_ROUND: 100, 2 * SCAN_ROUND + 2: 31}
CARRY_M = sum(CARRY_LISTS.values()) + 2 * SKIPPED   # 410


def scan_carry_case(d, seed=0):
    """(ids [CARRY_M], contrib [CARRY_M, d], prior grad [CARRY_N, d]) of an index that needs the scan's carry: lists (CARRY_LISTS: node
    -> length) on both sides of both round edges and nowhere else, so every list behind an edge begins where the rounds before it
    ended; two of them are longer than a wave, so their sorted copies are placed by the carry too.  Ids -1 and CARRY_N are skipped."""
    rng = np.random.default_rng(seed)
    ids = np.concatenate([np.full(k, v) for v, k in CARRY_LISTS.items()] + [np.full(SKIPPED, -1), np.full(SKIPPED, CARRY_N)]).astype(np.int32)
    rng.shuffle(ids)
    count = np.bincount(ids[(ids >= 0) & (ids < CARRY_N)], minlength=CARRY_N)
    assert len(ids) == CARRY_M and {int(v): int(count[v]) for v in np.nonzero(count)[0]} == CARRY_LISTS
    assert 2 * SCAN_ROUND < CARRY_N <= 3 * SCAN_ROUND and count[CARRY_HUB] > 64
    for edge in (SCAN_ROUND, 2 * SCAN_ROUND):       # a list ends the round before the edge, another begins the round behind it
        assert count[edge - 1] > 0 and count[edge] > 0 and count[:edge - 1].sum() > 0
    contrib = cancellation_lists(ids, CARRY_N, d, rng)
    grad = rng.standard_normal((CARRY_N, d)).astype(np.float32)
    return ids, contrib, grad
