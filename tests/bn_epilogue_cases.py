"""Cases, float64 reference, dropout-mask restatement and bounds for the fused BatchNorm1d + ReLU + dropout epilogue
(csrc/epilogue.hip: k_bn_partial, k_bn_final, k_bn_bwd_final, k_bn_apply) -- main.py:207-209.  Imports without a GPU:
test_bn_epilogue_cpu.py checks the reference against torch and runs a float32 restatement through the bounds,
test_bn_epilogue_f64_gpu.py runs the kernels through them.

Reference (NumPy float64 on the float32 inputs): mu, biased var, rstd = 1 / sqrt(var + eps); running statistics updated with
momentum and the unbiased variance (factor 1 for M = 1, as the kernel does); z = (x - mu) * rstd * gamma + beta;
y = mask * z / (1 - p) where z > 0; g = mask * dy / (1 - p) where z > 0; dbeta = sum g; dgamma = sum g * xhat;
dx = gamma * rstd * (g - mean g - xhat * mean(g * xhat)) in training mode, gamma * rstd * g with the running statistics in eval mode.

The dropout mask is restated from the kernel's contract (keep_mask below), not read back from y: a two-round fmix32 of the (low,
high) words of the seed and of the element index row * C + col, kept iff (h >> 8) >= threshold.

Bounds (a = |gamma| * rstd), from float32 rounding of the documented formulas and the float64 sums -- never from a kernel's output:
  save_mean   2^-23 |mu| (its rounding) + M 2^-52 mean|x| (worst case of a float64 sum of M terms)
  save_rstd   relative 2^-23 + M 2^-52 mean(x^2) / (var + eps): var = E[x^2] - E[x]^2 cancels numbers of size mean(x^2)
  running     running_mean: the save_mean bound + 2^-23 relative.  running_var: d var / var = -2 d rstd / rstd, so momentum *
              unbiased factor * 2 (var + eps) * (the save_rstd bound) + 2^-23 relative.
  z           2^-21 (|x - mu| a + |beta|) + 2^-22 |mu| a: x - mu32 carries mu's rounding (2^-24 |mu|), times rstd and gamma; the
              rest is a handful of float32 roundings of the two terms.  y: the same times 1 / (1 - p).
  dbeta, dgamma   sum |g| 2^-22 (1 + |xhat| + |mu| rstd) + 2^-24 |result|
  dx          2^-20 a (|g| + |mean g| + |xhat mean(g xhat)|) + 2^-22 a |mean(g xhat)| |mu| rstd
              + a (dbeta bound + |xhat| dgamma bound) / M
Two corrections of the first derivation, both found by the float32 restatement of test_bn_epilogue_cpu.py missing "half of the
bound" (no kernel output was involved):
  * the pure rounding terms of save_mean and the running statistics were 2^-24 relative.  That IS the worst case of one rounding to
    float32, so a correctly rounded result can sit at the bound itself (M = 1: nothing else contributes); they are one ulp, 2^-23.
  * dx had no term for the error of the two means it subtracts.  mean(g xhat) is a cancelling sum: its error is that of dgamma
    (governed by sum |g xhat|, not by the small result) divided by M, and it reaches dx times a |xhat|; likewise mean g.
Gate: an element whose reference |z| is below its z bound may fall on either side of the ReLU.  It is left out of the y and dx
checks, and what it could add to a column's sums -- |g| and |g xhat| of the kept ones, `amb_s` / `amb_q` -- is added to the dbeta /
dgamma bounds (and through them, divided by M, to the dx bounds of that column: the means that every dx of the column sees move
by that much).  The share of such elements is at most 1e-3 in every case (asserted on the CPU).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

EPS = 1e-5
MOMENTUM = 0.1
SENTINEL = np.float32(-12345.0)
EXCLUDED_CAP = 1e-3

PAIRS = ((1, 4), (1, 65), (2, 3), (2, 256), (15, 64), (15, 255), (16, 1), (16, 68), (17, 4), (17, 260), (33, 64), (33, 65), (33, 256),
         (4080, 4), (4081, 3), (4081, 4), (4097, 1), (4097, 68), (8209, 3), (8209, 4))
OFFSETS = (0.0, 1.0, 30.0, 100.0, 1000.0, -1000.0)


# ------------------------------------------------------------------------------------------------ the dropout mask

def _fmix32(h):
    m = np.uint64(0xffffffff)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85ebca6b)) & m
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xc2b2ae35)) & m
    return h ^ (h >> np.uint64(16))


def drop_threshold(p) -> int:
    p32 = np.float32(p)
    if not p32 > 0:
        return 0
    if p32 >= 1:
        return 1 << 24
    return int(np.float64(p32) * 16777216.0)


def keep_mask(seed: int, rows: int, cols: int, p, seed_dev: int = 0) -> np.ndarray:
    """bool [rows, cols]: element (r, c) is kept.  Index r * cols + c, seed = (seed + seed_dev) mod 2^64."""
    seed = (int(seed) + int(seed_dev)) % (1 << 64)
    m = np.uint64(0xffffffff)
    idx = np.arange(rows * cols, dtype=np.uint64)
    h = _fmix32((idx & m) ^ np.uint64(seed & 0xffffffff))
    h = _fmix32(h ^ (((idx >> np.uint64(32)) * np.uint64(0x9e3779b1)) & m) ^ np.uint64(seed >> 32))
    return ((h >> np.uint64(8)) >= np.uint64(drop_threshold(p))).reshape(rows, cols)


def inv_keep(training: bool, p) -> float:
    p32 = np.float32(p)
    return 1.0 / (1.0 - float(p32)) if training and 0 < p32 < 1 else 1.0


# ------------------------------------------------------------------------------------------------ cases

@dataclass
class BnCase:
    name: str
    x: np.ndarray                      # float32 [capacity, C]; rows past `rows` hold NaN and must not be read
    dy: np.ndarray
    gamma: np.ndarray
    beta: np.ndarray
    running_mean: np.ndarray
    running_var: np.ndarray
    training: bool
    p: float
    seed: int
    rows: int | None = None            # device extent (rows_dev); None: no extent, every row of x is real
    seed_dev: int | None = None
    no_running: bool = False           # running_mean / running_var NULL
    misalign: str | None = None        # "x", "gamma" or "save_mean": that operand starts one element into its buffer
    ext_rows_per_part: int | None = None   # the first stage of the statistics comes from outside (forward_stats)

    @property
    def m(self):
        return self.x.shape[0] if self.rows is None else self.rows


def _make(name, m, c, training, p, seed=0, x=None, **kw):
    rng = np.random.RandomState((m * 1000 + c + 17 * seed) % (2 ** 31))
    if x is None:
        x = rng.randn(m, c) * 2 + 0.7
    x = np.ascontiguousarray(x, dtype=np.float32)
    gamma = rng.uniform(0.5, 1.5, c)
    gamma[3::5] *= -1.0                                                # |gamma| in the bounds: some negative ones
    return BnCase(name, x, rng.randn(m, c).astype(np.float32), gamma.astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32),
                  rng.uniform(-1, 1, c).astype(np.float32), rng.uniform(0.5, 2, c).astype(np.float32), training, p,
                  seed=0x1234_5678_9abc_def0 + 977 * seed + m, **kw)


MODES = (("train p=0", True, 0.0), ("train p=0.5", True, 0.5), ("eval", False, 0.5))


def shape_cases():
    out = []
    for m, c in PAIRS:
        for label, training, p in MODES:
            out.append(_make(f"({m}, {c}) {label}", m, c, training, p))
    out.append(_make("(33, 64) train p=1", 33, 64, True, 1.0))
    out.append(_make("(33, 64) train p=0.5, no running statistics", 33, 64, True, 0.5, no_running=True))
    return out


def off_centre_x(m, c, seed):
    """Column j: spread 1, offset OFFSETS[j % 6]; the last column is constant."""
    rng = np.random.RandomState(seed)
    x = rng.randn(m, c) + np.array([OFFSETS[j % len(OFFSETS)] for j in range(c)])
    x[:, c - 1] = 3.0
    return x.astype(np.float32)


def off_centre_cases():
    out = []
    for m, c in ((8209, 8), (257, 256)):
        for label, training, p in MODES:
            out.append(_make(f"off-centre ({m}, {c}) {label}", m, c, training, p, seed=1, x=off_centre_x(m, c, m + c)))
    return out


def misaligned_cases():
    return [_make(f"misaligned {which} (33, 64) {label}", 33, 64, training, p, misalign=which)
            for which in (None, "x", "gamma", "save_mean") for label, training, p in MODES[1:]]


def extent_cases():
    out = []
    for cap, c, rows in ((4097, 64, 1), (4097, 64, 16), (4097, 64, 17), (4097, 64, 4096), (4097, 64, 4097), (33, 5, 20)):
        for label, training, p in MODES[1:]:
            case = _make(f"extent {rows} of ({cap}, {c}) {label}", cap, c, training, p, seed=rows, rows=rows,
                         seed_dev=0xffff_ffff_0000_0123 if rows == 17 else None)
            case.x[rows:] = np.nan
            case.dy[rows:] = np.nan
            out.append(case)
    return out


def external_cases():
    """sage_bn_relu_dropout_forward_stats: (rows_per_part, M, C); 9988 rows in tiles of 16 are 625 parts, more than BN_MAX_PARTS."""
    out = []
    for rpp, m, c in ((16, 9988, 8), (80, 200, 12), (16, 17, 5)):
        out.append(_make(f"external rows_per_part={rpp} ({m}, {c})", m, c, True, 0.5, seed=2, ext_rows_per_part=rpp))
    for rpp, cap, c, rows in ((16, 9988, 8, 9000), (80, 200, 12, 81)):
        case = _make(f"external rows_per_part={rpp} extent {rows} of ({cap}, {c})", cap, c, True, 0.5, seed=3, rows=rows, ext_rows_per_part=rpp)
        case.x[rows:] = np.nan
        case.dy[rows:] = np.nan
        out.append(case)
    return out


def external_partials(case: BnCase):
    """pa / pb [parts, C] float64: column sums of x and of x^2 per tile of rows_per_part rows, as the projection's epilogue leaves them;
    the tiles behind the true row count hold NaN (nobody wrote them)."""
    rpp, cap, c = case.ext_rows_per_part, case.x.shape[0], case.x.shape[1]
    parts = (cap + rpp - 1) // rpp
    pa, pb = np.full((parts, c), np.nan), np.full((parts, c), np.nan)
    x = case.x[:case.m].astype(np.float64)
    for t in range((case.m + rpp - 1) // rpp):
        tile = x[t * rpp:(t + 1) * rpp]
        pa[t], pb[t] = tile.sum(axis=0), (tile * tile).sum(axis=0)
    return pa, pb


FAMILIES = {"shapes": shape_cases, "off-centre": off_centre_cases, "misaligned": misaligned_cases, "extents": extent_cases,
            "external": external_cases}


# ------------------------------------------------------------------------------------------------ reference and bounds

@dataclass
class BnRef:
    mu: np.ndarray
    var: np.ndarray
    rstd: np.ndarray
    running_mean: np.ndarray | None
    running_var: np.ndarray | None
    y: np.ndarray
    dx: np.ndarray
    dbeta: np.ndarray
    dgamma: np.ndarray
    excluded: np.ndarray               # bool [M, C]
    on: np.ndarray                     # bool [M, C]: z > 0 and kept
    bounds: dict


def reference(case: BnCase) -> BnRef:
    m, c = case.m, case.x.shape[1]
    x = case.x[:m].astype(np.float64)
    dy = case.dy[:m].astype(np.float64)
    gamma, beta = case.gamma.astype(np.float64), case.beta.astype(np.float64)
    eps, mom = float(np.float32(EPS)), float(np.float32(MOMENTUM))
    rm, rv = case.running_mean.astype(np.float64), case.running_var.astype(np.float64)
    batch_mu, batch_var = x.mean(axis=0), x.var(axis=0)
    if case.training:
        mu, var = batch_mu, batch_var
        new_rm = (1 - mom) * rm + mom * mu
        factor = m / (m - 1) if m > 1 else 1.0
        new_rv = (1 - mom) * rv + mom * var * factor
    else:
        mu, var, new_rm, new_rv, factor = rm, rv, rm, rv, 1.0
    rstd = 1.0 / np.sqrt(var + eps)
    a = np.abs(gamma) * rstd
    xhat = (x - mu) * rstd
    z = xhat * gamma + beta
    keep = keep_mask(case.seed, m, c, case.p if case.training else 0.0, case.seed_dev or 0)
    ik = inv_keep(case.training, case.p)
    on = (z > 0) & keep
    y = np.where(on, z * ik, 0.0)
    g = np.where(on, dy * ik, 0.0)
    dbeta, dgamma = g.sum(axis=0), (g * xhat).sum(axis=0)
    k1, k2 = (dbeta / m, dgamma / m) if case.training else (np.zeros(c), np.zeros(c))
    dx = gamma * rstd * (g - k1 - xhat * k2)
    # bounds
    b = {}
    cond = m * 2.0 ** -52
    b["save_mean"] = 2.0 ** -23 * np.abs(mu) + cond * np.abs(x).mean(axis=0)
    b["save_rstd"] = (2.0 ** -23 + cond * (x * x).mean(axis=0) / (var + eps)) * rstd
    b["running_mean"] = b["save_mean"] + 2.0 ** -23 * np.abs(new_rm)
    b["running_var"] = mom * factor * 2.0 * (var + eps) * (b["save_rstd"] / rstd) + 2.0 ** -23 * np.abs(new_rv)
    zb = 2.0 ** -21 * (np.abs(x - mu) * a + np.abs(beta)) + 2.0 ** -22 * np.abs(mu) * a
    excluded = np.abs(z) < zb
    b["y"] = zb * ik
    gk = np.where(excluded & keep, np.abs(dy) * ik, 0.0)               # what an element on the gate could add to the sums
    amb_s, amb_q = gk.sum(axis=0), (gk * np.abs(xhat)).sum(axis=0)
    per = (np.abs(g) * 2.0 ** -22 * (1.0 + np.abs(xhat) + np.abs(mu) * rstd)).sum(axis=0)
    b["grad_beta"] = per + 2.0 ** -24 * np.abs(dbeta) + amb_s
    b["grad_gamma"] = per + 2.0 ** -24 * np.abs(dgamma) + amb_q
    b["grad_x"] = (2.0 ** -20 * a * (np.abs(g) + np.abs(k1) + np.abs(xhat * k2)) + 2.0 ** -22 * a * np.abs(k2) * np.abs(mu) * rstd
                   + (a * (b["grad_beta"] + np.abs(xhat) * b["grad_gamma"]) / m if case.training else 0.0))
    no_run = case.no_running
    return BnRef(mu, var, rstd, None if no_run else new_rm, None if no_run else new_rv, y, dx, dbeta, dgamma, excluded, on, b)


def restate32(case: BnCase) -> dict:
    """The documented formulas in NumPy float32 (float64 only where the kernels use it: the column sums and what is formed from
    them before the one rounding to float32), in the shape of the GPU test's output: what a correct float32 implementation returns."""
    f = np.float32
    m, c, cap = case.m, case.x.shape[1], case.x.shape[0]
    x, dy = case.x[:m], case.dy[:m]
    eps, mom = float(f(EPS)), float(f(MOMENTUM))
    rm, rv = case.running_mean.copy(), case.running_var.copy()
    if case.training:
        x64 = x.astype(np.float64)
        mu = x64.sum(axis=0) / m
        var = np.maximum((x64 * x64).sum(axis=0) / m - mu * mu, 0.0)
        mean32, rstd32 = mu.astype(f), (1.0 / np.sqrt(var + eps)).astype(f)
        unbiased = var * (m / (m - 1)) if m > 1 else var
        rm = ((1 - mom) * rm.astype(np.float64) + mom * mu).astype(f)
        rv = ((1 - mom) * rv.astype(np.float64) + mom * unbiased).astype(f)
    else:
        mean32, rstd32 = rm.copy(), (1.0 / np.sqrt(rv.astype(np.float64) + eps)).astype(f)
    xhat = (x - mean32) * rstd32
    z = xhat * case.gamma + case.beta
    assert xhat.dtype == f and z.dtype == f
    ik = f(inv_keep(case.training, case.p))
    on = (z > 0) & keep_mask(case.seed, m, c, case.p if case.training else 0.0, case.seed_dev or 0)
    g = np.where(on, dy * ik, f(0))
    s, q = g.astype(np.float64).sum(axis=0), (g.astype(np.float64) * xhat.astype(np.float64)).sum(axis=0)
    c1, c2 = ((s / m).astype(f), (q / m).astype(f)) if case.training else (np.zeros(c, f), np.zeros(c, f))
    y, gx = np.full((cap, c), SENTINEL), np.full((cap, c), SENTINEL)
    y[:m] = np.where(on, z * ik, f(0))
    gx[:m] = case.gamma * rstd32 * (g - c1 - xhat * c2)
    return {"save_mean": mean32, "save_rstd": rstd32, "running_mean": None if case.no_running else rm,
            "running_var": None if case.no_running else rv, "y": y, "grad_x": gx, "grad_beta": s.astype(f), "grad_gamma": q.astype(f)}


def check(case: BnCase, ref: BnRef, got: dict, limit: float = 1.0) -> dict:
    """Assert the outputs of one forward + backward call against the reference; return the worst error-to-bound ratio per output."""
    m = case.m
    ratios = {}

    def close(key, value, want, bound, where=None):
        err = np.abs(np.asarray(value, dtype=np.float64) - want)
        assert np.isfinite(err).all(), (case.name, key, "non-finite output")
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0.0, 0.0, err / bound)
        if where is not None:
            r = np.where(where, r, 0.0)
        ratios[key] = float(r.max())
        assert ratios[key] <= limit, (case.name, key, ratios[key], np.unravel_index(int(r.argmax()), r.shape))

    close("save_mean", got["save_mean"], ref.mu, ref.bounds["save_mean"])
    close("save_rstd", got["save_rstd"], ref.rstd, ref.bounds["save_rstd"])
    if ref.running_mean is not None:
        if case.training:
            close("running_mean", got["running_mean"], ref.running_mean, ref.bounds["running_mean"])
            close("running_var", got["running_var"], ref.running_var, ref.bounds["running_var"])
        else:
            assert np.array_equal(got["running_mean"], case.running_mean) and np.array_equal(got["running_var"], case.running_var), case.name
    y, gx = np.asarray(got["y"]), np.asarray(got["grad_x"])
    assert y.shape == case.x.shape and gx.shape == case.x.shape
    assert np.all(y[m:] == SENTINEL) and np.all(gx[m:] == SENTINEL), (case.name, "a row past the true count was written")
    check_at = ~ref.excluded
    assert not y[:m][check_at & ~ref.on].any(), (case.name, "y is not exactly zero where the mask or the ReLU closes")
    close("y", y[:m], ref.y, ref.bounds["y"], check_at)
    close("grad_x", gx[:m], ref.dx, ref.bounds["grad_x"], check_at)
    close("grad_beta", got["grad_beta"], ref.dbeta, ref.bounds["grad_beta"])
    close("grad_gamma", got["grad_gamma"], ref.dgamma, ref.bounds["grad_gamma"])
    return ratios


def merge(into: dict, ratios: dict) -> None:
    for k, v in ratios.items():
        into[k] = max(into.get(k, 0.0), v)
