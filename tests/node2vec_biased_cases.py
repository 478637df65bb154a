"""Shared by tests/test_node2vec_biased_cpu.py and tests/test_node2vec_biased_gpu.py (no tests here): a NumPy restatement of
pope_n2v_walks_biased as include/graphpope_hip.h states it -- uint64 arithmetic with overflow ignored, float64 comparisons -- which
also counts the steps that reached the exact pass; a restatement of the first-order rule written on its own; and the graphs.

The restatement is vectorised over the walks for the 16 rejection tries and goes walk by walk through the exact pass, where
``np.cumsum`` adds the weights in slot order one after the other, as the kernel does."""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
D = np.uint64(0xD1B54A32D192ED03)
TRIES = 16
TWO32 = 4294967296.0
MASK64 = (1 << 64) - 1


def _u64(a):
    return np.atleast_1d(np.asarray(a)).astype(np.uint64)


def mix64(z):
    """The splitmix64 finaliser on a uint64 array."""
    z = _u64(z)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def below(draw, n):
    """(draw * n) >> 32 for 32-bit draws and n < 2^31, as int64."""
    return ((_u64(draw) * _u64(n)) >> np.uint64(32)).astype(np.int64)


def row_keys(seed, first_row, b):
    rows = _u64(first_row + np.arange(b, dtype=np.int64))
    return mix64(_u64(seed & MASK64) + G * (np.uint64(2) * rows + np.uint64(1)))


def draw(step_key, j, which):
    return mix64(step_key + G * _u64(2 * j + which)) >> np.uint64(32)


def canonical_csr(ei, n):
    """(rowptr int64 [n + 1], col int64 [E]): rows by source, every row's targets ascending, repeated edges kept."""
    ei = np.asarray(ei, dtype=np.int64)
    order = np.lexsort((ei[1], ei[0]))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ei[0], minlength=n), out=rowptr[1:])
    return rowptr, ei[1][order]


def walks_biased_ref(rowptr, col, n, starts, length, seed, p, q, first_row=0):
    """(pos int64 [B, length + 1], the number of steps that reached the exact pass)."""
    rowptr, col, starts = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(starts, dtype=np.int64)
    b = starts.shape[0]
    inv_p, inv_q = 1.0 / float(p), 1.0 / float(q)
    w_max = max(inv_p, 1.0, inv_q)
    edge_keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr)) * n + col[:rowptr[n]]
    assert (np.diff(edge_keys) >= 0).all(), "every CSR row must be ascending"

    def weight(t, x):                                   # x == t: 1 / p; t -> x an edge: 1; else 1 / q
        k = t * n + x
        at = np.minimum(np.searchsorted(edge_keys, k), max(len(edge_keys) - 1, 0))
        return np.where(x == t, inv_p, np.where(edge_keys[at] == k, 1.0, inv_q))

    key_of_row = row_keys(seed, first_row, b)
    valid = (starts >= 0) & (starts < n)
    cur, t = np.where(valid, starts, 0), np.zeros(b, dtype=np.int64)
    pos = np.empty((b, length + 1), dtype=np.int64)
    pos[:, 0] = starts
    exact = 0
    with np.errstate(over="ignore"):
        for s in range(length):
            lo = rowptr[cur]
            deg = rowptr[cur + 1] - lo
            move = valid & (deg > 0)
            key = key_of_row ^ (D * _u64(s + 1))
            nxt = cur.copy()
            if s == 0:
                i = np.nonzero(move)[0]
                nxt[i] = col[lo[i] + below(draw(key[i], 0, 0), deg[i])]
            else:
                pending = move.copy()
                for j in range(TRIES):
                    i = np.nonzero(pending)[0]
                    if i.size == 0:
                        break
                    x = col[lo[i] + below(draw(key[i], j, 0), deg[i])]
                    ok = draw(key[i], j, 1).astype(np.float64) * w_max < weight(t[i], x) * TWO32
                    nxt[i[ok]] = x[ok]
                    pending[i[ok]] = False
                for i in np.nonzero(pending)[0]:
                    exact += 1
                    xs = col[lo[i]:lo[i] + deg[i]]
                    prefix = np.cumsum(weight(np.full(xs.shape, t[i]), xs))                 # in slot order, float64
                    target = float(draw(key[i:i + 1], TRIES, 0)[0]) * (1.0 / TWO32) * prefix[-1]
                    above = np.nonzero(prefix > target)[0]
                    nxt[i] = xs[above[0] if above.size else deg[i] - 1]
            t = np.where(move, cur, t)
            cur = np.where(move, nxt, cur)
            pos[:, s + 1] = np.where(valid, cur, starts)
    return pos, exact


def walks_first_order_ref(rowptr, col, n, starts, length, seed, first_row=0):
    """pope_n2v_walks' positive rows, written from its own statement: one draw per (row, step), keyed on (seed, row, step, kind 0)."""
    pos = np.empty((len(starts), length + 1), dtype=np.int64)
    with np.errstate(over="ignore"):
        for i, start in enumerate(np.asarray(starts, dtype=np.int64)):
            row_key = mix64(_u64(seed & MASK64) + G * _u64(2 * (first_row + i) + 0 + 1))
            cur = int(start)
            pos[i, 0] = cur
            for s in range(length):
                if 0 <= start < n and rowptr[cur + 1] > rowptr[cur]:
                    d32 = mix64(row_key ^ (D * _u64(s + 1))) >> np.uint64(32)
                    cur = int(col[rowptr[cur] + int(below(d32, rowptr[cur + 1] - rowptr[cur])[0])])
                pos[i, s + 1] = cur
    return pos


# ---- graphs ------------------------------------------------------------------------------------------------------------------
N70, L7, C4 = 70, 7, 4


def graph70():
    """The graph of tests/test_node2vec_gpu.py.  70 nodes, directed.  0: hub of out-degree 100 (every target 10..59 twice).  1:
    out-degree 0 with in-edges.  3: self-loop.  4 -> 5 twice.  7 <-> 8: a 2-node cycle with no other way out.  69: isolated.  The
    rest: a ring with chords."""
    e = [(0, 10 + t % 50) for t in range(100)]
    e += [(2, 1), (2, 3), (3, 3), (3, 1), (3, 4), (4, 5), (4, 5), (4, 6), (5, 0), (6, 4), (6, 2), (7, 8), (8, 7), (9, 7), (9, 10)]
    for v in range(10, 69):
        e += [(v, 10 + (v - 9) % 59), (v, 10 + (v * 7) % 59)]
        if v % 5 == 0:
            e.append((v, (1, 7, 3, 4, 0, 9, 2)[(v // 5) % 7]))
    ei = np.array(e, dtype=np.int64).T
    return ei[:, np.random.default_rng(0).permutation(ei.shape[1])]              # not sorted by source


def starts201():
    s = (np.arange(201, dtype=np.int64) * 37) % N70                               # every node, with repeats; 201 is no multiple of 64
    s[:6] = [7, 8, 1, 69, 0, 3]
    return s


PQ70 = [(0.25, 4.0), (4.0, 0.25), (2.0, 1.0), (1.0, 0.5), (1e6, 1.0), (1.0, 1e6)]
SEED70 = 11

N_FAN = 9


def fan_graph():
    """0 -> {1, 2, 3, 4}; 1 -> {0, 2, ..., 8}; x -> 0 for x = 2..8.  After 0 -> 1 the second step sees one return (0), three
    out-neighbours of 0 (2, 3, 4) and four nodes at distance 2 (5..8); from 2..4 the only way is back."""
    e = [(0, x) for x in (1, 2, 3, 4)] + [(1, 0)] + [(1, x) for x in range(2, 9)] + [(x, 0) for x in range(2, 9)]
    return np.array(e, dtype=np.int64).T


FAN_B = 65536
FAN_SEEDS = [20260101, 1, 2, 3]
# (p, q) -> the unnormalised weights of the second step from t = 0, v = 1 over the targets 0, 2, 3, ..., 8
FAN_WEIGHTS = {(4.0, 0.5): [0.25, 1, 1, 1, 2, 2, 2, 2], (0.25, 2.0): [4, 1, 1, 1, 0.5, 0.5, 0.5, 0.5]}
FAN_RUNS = [(p, q, seed) for (p, q) in FAN_WEIGHTS for seed in FAN_SEEDS]


def fan_second_step_deviation(pos, p, q):
    """Among the walks whose first step is 1: the largest |count - expectation| / sigma over the eight second-step targets, sigma that
    of a binomial count; and the number of such walks."""
    pos = np.asarray(pos)
    second = pos[pos[:, 1] == 1][:, 2]
    m = second.shape[0]
    w = np.array(FAN_WEIGHTS[p, q], dtype=np.float64)
    prob = w / w.sum()
    counts = np.bincount(second, minlength=N_FAN)[[0, 2, 3, 4, 5, 6, 7, 8]]
    assert counts.sum() == m                                                     # nothing went to node 1 itself
    sigma = np.sqrt(m * prob * (1 - prob))
    return float((np.abs(counts - m * prob) / sigma).max()), m


def community_graph(seed, n=512, communities=4):
    """The graph of tests/test_node2vec_gpu.py's training test.  label = v % 4.  For v in order: 8 targets with replacement from v's
    community, then 1 from the others; self-loops dropped, both directions added, duplicates removed."""
    rng = np.random.default_rng(seed)
    nodes = np.arange(n)
    src, dst = [], []
    for v in range(n):
        same = nodes[nodes % communities == v % communities]
        other = nodes[nodes % communities != v % communities]
        t = np.concatenate([rng.choice(same, 8), rng.choice(other, 1)])
        src.append(np.full(9, v))
        dst.append(t)
    src, dst = np.concatenate(src), np.concatenate(dst)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    key = np.unique(np.concatenate([src * n + dst, dst * n + src]))
    return np.stack([key // n, key % n]).astype(np.int64)


def centroid_accuracy(table, n=512, communities=4):
    """Nearest-centroid accuracy on the odd half, centroids of the normalised rows fitted on the even half (float64, NumPy)."""
    z = np.asarray(table, dtype=np.float64)
    z = z / np.maximum(np.linalg.norm(z, axis=1, keepdims=True), 1e-12)
    v = np.arange(n)
    label, fit_half = v % communities, (v // communities) % 2 == 0
    centroids = np.stack([z[fit_half & (label == c)].mean(0) for c in range(communities)])
    pred = (z[~fit_half] @ centroids.T).argmax(1)
    return float((pred == label[~fit_half]).mean())
