"""Shared by tests/test_deterministic_cpu.py and tests/test_deterministic_gpu.py: the contract of sage_scatter_mean_det
(include/graphpope_hip.h) restated as a NumPy float32 loop, and the hand-built block the GPU tests run.  Not a test module."""
import numpy as np

N_DST, N_SRC = 130, 200
HUB, IN64, IN65 = 150, 5, 160                       # sources listed by 129, 64 and 65 destinations
IN1_LOW, IN1_HIGH, TWICE = 7, 170, 8                # in-degree 1 below / behind the destinations; listed twice by ONE destination
IN0_LOW, IN0_HIGH = 6, 199                          # never listed
DEG0, DEG64, DEG65, DEG_TWICE = 0, 10, 11, 12       # destinations of degree 0, 64, 65, and the one that lists TWICE twice


def scatter_mean_reference(rowptr, col, n_src, n_dst, gagg, gx):
    """The contract, term by term: every product grad_agg[i] * (1 / deg_i) rounded to float32, then added to the source's row in
    ascending slot order (one float32 addition each, no fused multiply-add: NumPy has none).  Rows [n_dst, n_src) start from +0."""
    out = np.zeros((n_src, gagg.shape[1]), dtype=np.float32)
    out[:n_dst] = gx[:n_dst]
    for i in range(n_dst):
        beg, end = int(rowptr[i]), int(rowptr[i + 1])
        if end == beg:
            continue
        term = gagg[i] * (np.float32(1.0) / np.float32(end - beg))
        assert term.dtype == np.float32
        for p in range(beg, end):                    # ascending p over the whole block = ascending p inside every source's list
            out[col[p]] = out[col[p]] + term
    return out


def hand_built_block():
    """(rowptr, col) of a block with N_DST destinations and N_SRC sources that holds every list length the sum kernel treats
    differently: sources with 0, 1, 2 (one destination twice), 64, 65 and 129 entries, destinations with 0, 1, 64 and 65."""
    named = {HUB, IN64, IN65, IN1_LOW, IN1_HIGH, TWICE, IN0_LOW, IN0_HIGH}
    fillers = [j for j in range(N_SRC) if j not in named]
    rows = [[] for _ in range(N_DST)]
    for i in range(1, N_DST):
        rows[i].append(HUB)
    for i in range(1, 65):
        rows[i].append(IN64)
    for i in range(1, 66):
        rows[i].append(IN65)
    rows[3].append(IN1_LOW)
    rows[4].append(IN1_HIGH)
    rows[DEG_TWICE] += [TWICE, fillers[0], TWICE]
    rs = np.random.RandomState(5)
    for i, want in ((DEG64, 64), (DEG65, 65)):
        rows[i] += list(rs.choice(fillers, size=want - len(rows[i]), replace=False))
    for r in rows:                                   # the hub does not come first in every row
        rs.shuffle(r)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.array([j for r in rows for j in r], dtype=np.int32)
    # the block has what it was built for
    deg, in_deg = np.diff(rowptr), np.bincount(col, minlength=N_SRC)
    assert deg[DEG0] == 0 and deg[DEG64] == 64 and deg[DEG65] == 65 and (deg[66:] == 1).all()
    assert in_deg[HUB] == 129 and in_deg[IN64] == 64 and in_deg[IN65] == 65 and in_deg[IN1_LOW] == 1 and in_deg[IN1_HIGH] == 1
    assert in_deg[IN0_LOW] == 0 and in_deg[IN0_HIGH] == 0 and in_deg[TWICE] == 2 and list(col[rowptr[12]:rowptr[13]]).count(TWICE) == 2
    assert IN0_LOW < N_DST <= IN0_HIGH and IN1_LOW < N_DST <= IN1_HIGH
    return rowptr, col


def random_block(n_dst, n_src, seed):
    """Degrees 0 .. 9 and three rows of 70 (lists longer than a wave appear at source 0, which half of all slots name)."""
    rs = np.random.RandomState(seed)
    deg = rs.randint(0, 10, size=n_dst)
    deg[rs.choice(n_dst, size=3, replace=False)] = 70
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = rs.randint(0, n_src, size=int(rowptr[-1])).astype(np.int32)
    col[rs.rand(len(col)) < 0.5] = 0
    return rowptr, col


SCAN_ROUND = 8192                                    # entries the one-block scan of the index takes per round (1024 threads x 8)
CARRY_N_DST, CARRY_N_SRC = 96, 2 * SCAN_ROUND + 3    # three rounds, the last with 3 entries
CARRY_HUB = SCAN_ROUND                               # the first source of round 1, listed by 70 destinations
CARRY_LISTS = {0: 3, SCAN_ROUND - 1: 5, CARRY_HUB: 70, 2 * SCAN_ROUND - 1: 2, 2 * SCAN_ROUND: 4, 2 * SCAN_ROUND + 2: 1}


def scan_carry_block():
    """(rowptr, col) of a block whose index needs the scan's carry: CARRY_N_SRC sources, lists (CARRY_LISTS: source -> length) on
    both sides of both round edges and nowhere else, so every list behind an edge begins where the rounds before it ended; the list
    at CARRY_HUB is longer than a wave, so its sorted copy is placed by the carry too."""
    rs = np.random.RandomState(11)
    rows = [[] for _ in range(CARRY_N_DST)]
    for j, length in CARRY_LISTS.items():
        for i in rs.choice(CARRY_N_DST - 1, size=length, replace=False):       # (the last destination keeps degree 0)
            rows[i].append(j)
    for r in rows:
        rs.shuffle(r)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.array([j for r in rows for j in r], dtype=np.int32)
    in_deg = np.bincount(col, minlength=CARRY_N_SRC)
    assert len(in_deg) == CARRY_N_SRC and {int(j): int(in_deg[j]) for j in np.nonzero(in_deg)[0]} == CARRY_LISTS
    assert 2 * SCAN_ROUND < CARRY_N_SRC <= 3 * SCAN_ROUND and in_deg[CARRY_HUB] > 64
    for edge in (SCAN_ROUND, 2 * SCAN_ROUND):        # a list ends the round before the edge, another begins the round behind it
        assert in_deg[edge - 1] > 0 and in_deg[edge] > 0 and in_deg[:edge - 1].sum() > 0
    return rowptr, col
