"""Off-centre tables for the node2vec-space path (csrc/pairwise.hip, csrc/pairwise_persistent.h), NumPy only.

The euclidean epilogue forms d2 = |x|^2 + |a|^2 - 2 x.a in float32 and recomputes an output as a direct sum of squared
differences where d2 < CANCEL_RATIO * (|x|^2 + |a|^2).  Rows that share an offset mu per component (spread sigma = 1) have
d2 / norms ~ 1 / (mu^2 + 1), so mu chooses the regime: far above the threshold, just above it (the fast path is trusted
although it has lost digits), straddling it (both paths inside one tile) or below it everywhere (the wave-wide fix-up
runs for every output, ragged tiles included).

Anchors are rows of the table (without replacement, plus one repeated id): every column holds its anchor's own row, the
column minimum of `euclidean` and `distance` is 0 and the float32 MinMaxScaler arithmetic adds at most one ulp of 1.  With
anchors that are not table rows the reference's own float32 scaling would exceed the 1e-5 gate and prove nothing.

Used by test_pairwise_cases_cpu.py (the conditions that keep the GPU tests honest), test_pairwise_conditioning_gpu.py and
tools/pairwise_conditioning_table.py.
"""
import functools
import math
from collections import namedtuple

import numpy as np

# The kernel's cancellation threshold: PW_CANCEL_RATIO in csrc/pairwise_epilogue.h (the metric epilogue of k_pairwise and
# k_pairwise_persistent).  The mu values of the `straddle` and `just_above` cases follow from it; if the kernel constant
# moves, move this value with it and they follow.
CANCEL_RATIO = 0.125
JUST_ABOVE_MAX = 5 * CANCEL_RATIO            # `just_above`: ratio in (CANCEL_RATIO, JUST_ABOVE_MAX]
# `far`: every non-coincident pair above it -- five thresholds, but no more than 0.3: the expansion then loses less than
# two bits whatever the threshold is, and a zero-mean table has pairs down to 0.38 (D = 36)
FAR_RATIO = min(5 * CANCEL_RATIO, 0.3)
EPS32 = float(np.finfo(np.float32).eps)
FNS = ("euclidean", "distance", "similarity")


def mu_for_ratio(ratio):
    """The offset per component (sigma = 1) whose expected d2 / norms is `ratio`: 1 / (mu^2 + 1) = ratio."""
    return math.sqrt(1.0 / ratio - 1.0)


MU_STRADDLE = math.floor(10 * mu_for_ratio(CANCEL_RATIO)) / 10          # 2.6 for 2^-3 (9.9 for 1e-2): about half of the pairs on either side
MU_JUST_ABOVE = (round(mu_for_ratio(2.7 * CANCEL_RATIO), 1),            # 1.4 and 2.0 for 2^-3 (6 and 8 for 1e-2): 2.7 x and 1.54 x the threshold
                 round(mu_for_ratio(1.54 * CANCEL_RATIO), 1))

Case = namedtuple("Case", "name n k d mu seed regime")


def regime_of(mu):
    """The regime a table of offset mu is CLAIMED to be in (test_pairwise_cases_cpu.py checks the claim against ratio64);
    None: between two regimes, run for its error only."""
    if mu == MU_STRADDLE:
        return "straddle"
    if mu in MU_JUST_ABOVE:
        return "just_above"
    r = 1.0 / (mu * mu + 1.0)
    if r >= min(10 * CANCEL_RATIO, 1.0):
        return "far"
    if r <= 0.7 * CANCEL_RATIO:
        return "all_below"
    return None


def _case(n, k, d, mu):
    regime = regime_of(mu)
    seed = 100000 * (k % 7) + 1000 * d + int(round(10 * mu))       # of the shape and the offset, not of the place in the list
    return Case(f"n{n}_k{k}_d{d}_mu{mu:g}_{regime or 'between'}", n, k, d, float(mu), seed, regime)


def _mus(fixed):
    return sorted(set(fixed) | {MU_STRADDLE} | set(MU_JUST_ABOVE[:1]))


# N = 700: 21 whole 32-row tiles + 28 rows (persistent kernel), 10 whole 64-row tiles + 60 rows (k_pairwise).
# K = 65: one live column in the second 64-column wave -- the wave-wide fix-up runs with dead lanes.
N, K = 700, 65
CASES = [_case(N, K, 128, mu) for mu in sorted(set([0, 2, 4, 6, 8, 9, 9.9, 12, 30]) | {MU_STRADDLE} | set(MU_JUST_ABOVE))]
# D = 36, 100: short rows, zero-padded in LDS.  132: above the persistent kernel's depth, 16-byte rows (vector layout of
# k_pairwise).  129: generic layout, scalar k_sqnorm.  260: more than two 128-deep slabs.
for _d in (36, 100, 132, 129, 260):
    CASES += [_case(N, K, _d, mu) for mu in _mus([0, 6, 9.9, 30])]
# two column groups of the persistent kernel, the last one with ONE column; a table smaller than two tiles
for _mu in sorted({9.9, MU_STRADDLE}):
    CASES.append(_case(N, 257, 128, _mu))
    CASES.append(_case(33, 5, 4, _mu))
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def offset_table(n, d, mu, seed):
    return (mu + np.random.RandomState(seed).randn(n, d)).astype(np.float32)


def anchor_ids(n, k, seed):
    """k - 1 distinct rows and one of them again, in a seeded order."""
    rs = np.random.RandomState(seed + 77)
    ids = rs.choice(n, k - 1, replace=False)
    ids = np.append(ids, ids[rs.randint(k - 1)])
    return ids[rs.permutation(k)].astype(np.int64)


def ref64(emb, anchors, fn):
    """The raw [N, K] matrix in float64.  euclidean: square root of the direct sum of squared differences (no expansion);
    cosine: f64 norms, zero norms replaced by 1; `distance` clipped to [0, 2]."""
    x = np.asarray(emb, dtype=np.float64)
    a = x[np.asarray(anchors)] if np.ndim(anchors) == 1 else np.asarray(anchors, dtype=np.float64)
    if fn == "euclidean":
        out = np.empty((x.shape[0], a.shape[0]))
        for j in range(a.shape[0]):
            diff = x - a[j]
            out[:, j] = np.sqrt(np.einsum("ij,ij->i", diff, diff))
        return out
    nx, na = np.sqrt(np.einsum("ij,ij->i", x, x)), np.sqrt(np.einsum("ij,ij->i", a, a))
    nx[nx == 0.0] = 1.0
    na[na == 0.0] = 1.0
    sim = (x @ a.T) / nx[:, None] / na[None, :]
    if fn == "similarity":
        return sim
    if fn == "distance":
        return np.clip(1.0 - sim, 0.0, 2.0)
    raise KeyError(fn)


def scale64(raw):
    """Per-column min-max in float64 with the reference's rule for constant columns (range < 10 eps32 -> 1)."""
    raw = np.asarray(raw, dtype=np.float64)
    mn = raw.min(axis=0)
    rng = raw.max(axis=0) - mn
    rng = np.where(rng < 10 * EPS32, 1.0, rng)
    return (raw - mn) / rng


def ratio64(emb, anchors):
    """d2 / (|x|^2 + |a|^2) in float64, [N, K]: what the kernel's threshold is compared with."""
    x = np.asarray(emb, dtype=np.float64)
    a = x[np.asarray(anchors)]
    d = ref64(emb, anchors, "euclidean")
    norms = np.einsum("ij,ij->i", x, x)[:, None] + np.einsum("ij,ij->i", a, a)[None, :]
    return d * d / norms


def coincident(emb, anchors):
    """[N, K] bool: the row IS the anchor row (same id, or equal contents)."""
    emb = np.asarray(emb)
    return (emb[:, None, :] == emb[np.asarray(anchors)][None, :, :]).all(axis=2)


Inputs = namedtuple("Inputs", "case emb anchors")


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = CASE_BY_NAME[name]
    emb = offset_table(c.n, c.d, c.mu, c.seed)
    emb.setflags(write=False)
    anchors = anchor_ids(c.n, c.k, c.seed)
    anchors.setflags(write=False)
    return Inputs(c, emb, anchors)


@functools.lru_cache(maxsize=None)
def want64(name, fn):
    """scale64(ref64) of a case: computed once, shared by every test that needs it, read-only."""
    i = inputs(name)
    w = scale64(ref64(i.emb, i.anchors, fn))
    w.setflags(write=False)
    return w


def features(n, f, seed=5):
    return np.random.RandomState(seed).rand(n, f).astype(np.float32)


def degenerate_table(d, seed=4000):
    """A zero-mean table with an exact zero row (row 3), a row of components 1e-25 whose squares underflow float32 (row 11),
    and both among the anchors.  The reference treats both as zero rows: similarity 0, distance 1."""
    emb = offset_table(N, d, 0.0, seed + d)
    emb[3] = 0.0
    emb[11] = np.float32(1e-25)
    anchors = anchor_ids(N, K, seed + d)
    keep = anchors[~np.isin(anchors, (3, 11))]
    anchors = np.concatenate([[3, 11], keep])[:K].astype(np.int64)
    anchors[-1] = 3                                   # the zero row twice: once in each 64-column wave
    return emb, anchors
