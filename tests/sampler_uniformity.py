"""Chi-square statistics for the fan-out sampler's draw, shared by tests/test_oracle.py (the CPU restatement's permutation)
and tests/test_sampler_gpu.py (the HIP kernel).  Nothing here knows how the draw is made: the input is a table of picks.

A row with d neighbours and fan-out f < d must get a uniformly random ordered f-subset of [0, d).  Over S independent rows:

* inclusion counts c_v (how often neighbour v was picked at all): every c_v is Binomial(S, f/d) and the counts sum to S f,
  so Q = sum((c_v - S f/d)^2) / (S (f/d)(1 - f/d)) * (d-1)/d is chi-square on d-1 degrees of freedom;
* slot 0 alone is a uniform draw from [0, d): Pearson's chi-square on d-1 degrees of freedom;
* the ordered pair (slot 0, slot 1) is uniform over the d(d-1) ordered pairs of distinct values: Pearson's chi-square on
  d(d-1)-1 degrees of freedom (only for d <= 17, where S / (d(d-1)) keeps the expected cell count at 15 or more).

The bound is the chi-square critical value at an upper tail of 1e-4: it comes from the distribution and from nothing in this
project.  The inputs are fixed, so a test built on this is deterministic.
"""
import numpy as np
from scipy.stats import chi2

TAIL = 1.0e-4
# (d, fan-out): Feistel half widths 1..6, d on both sides of every power of two that changes the width, the project's own
# fan-outs 25 and 10 just below d, and small subsets of small rows (where a 4-round network was measurably biased)
CASES = [(3, 1), (3, 2), (4, 2), (5, 2), (5, 4), (6, 3), (8, 3), (9, 2), (11, 10), (13, 10), (16, 10), (17, 10), (26, 25), (40, 25),
         (64, 25), (65, 25), (100, 10), (257, 25), (1025, 10)]
SEEDS = [1, 2**40 + 7]
PAIR_MAX_D = 17


def inclusion_chi_square(counts, n_rows, fanout):
    """Q of the inclusion counts `counts` (one per neighbour) over n_rows draws of `fanout` distinct neighbours."""
    counts = np.asarray(counts, np.float64)
    d = len(counts)
    q = fanout / d
    return float(((counts - n_rows * q) ** 2).sum() / (n_rows * q * (1.0 - q)) * (d - 1) / d), d - 1


def statistics(picks, d, pair=None):
    """[(name, Q, degrees of freedom)] for picks [S, f]: row s holds the f distinct values of [0, d) drawn for row s, in slot order.
    pair: include the ordered-pair statistic (default: for d <= PAIR_MAX_D; the caller needs S / (d(d-1)) of 5 or more)."""
    picks = np.asarray(picks, np.int64)
    n_rows, f = picks.shape
    assert picks.min() >= 0 and picks.max() < d
    ordered = np.sort(picks, axis=1)
    assert (ordered[:, 1:] != ordered[:, :-1]).all(), "a row repeats a neighbour"
    out = [("inclusion",) + inclusion_chi_square(np.bincount(picks.ravel(), minlength=d), n_rows, f)]
    slot0 = np.bincount(picks[:, 0], minlength=d).astype(np.float64)
    out.append(("slot0", float(((slot0 - n_rows / d) ** 2).sum() / (n_rows / d)), d - 1))
    if f >= 2 and (d <= PAIR_MAX_D if pair is None else pair):
        pair = np.bincount(picks[:, 0] * d + picks[:, 1], minlength=d * d).reshape(d, d).astype(np.float64)
        e = n_rows / (d * (d - 1))
        out.append(("pair", float(((pair[~np.eye(d, dtype=bool)] - e) ** 2).sum() / e), d * (d - 1) - 1))
    return out


def critical(dof):
    return float(chi2.isf(TAIL, dof))


def assert_uniform(picks, d, what, pair=None):
    """Every statistic of `picks` below its critical value; prints each figure first (pytest -s / -rA shows them)."""
    stats = statistics(picks, d, pair)
    for name, q, dof in stats:
        print(f"{what}: {name} chi2 = {q:.1f} on {dof} dof, critical {critical(dof):.1f}, p = {chi2.sf(q, dof):.3g}")
    bad = [(name, round(q, 1), dof, round(critical(dof), 1)) for name, q, dof in stats if not q < critical(dof)]
    assert not bad, f"{what}: not uniform (statistic, chi2, dof, critical value at {TAIL}): {bad}"
