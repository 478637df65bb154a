"""Cases, float64 reference, float32 restatement and rounding bounds for the row L2 normalisation (include/graphpope_hip.h:
sage_l2_normalize_forward / _backward; PyG SAGEConv(normalize=True): F.normalize(out, p=2., dim=-1)).  Imports without a GPU and is not a
test module: test_l2norm_cpu.py proves the reference and the bounds on the CPU, test_l2norm_gpu.py runs the kernels through them.

Reference (:func:`reference`): NumPy float64 on the float32 inputs.
    n = sqrt(sum_c x_c^2),  t = max(n, eps),  y = x / t,  inv = 1 / t
    where n >= eps:  gx = (g - y (y . g)) / t            where n < eps (the clamp branch; an all-zero row too):  gx = g / eps
eps is the float32 nearest 1e-12, the number the kernels are handed.

Bounds, from float32 rounding alone (u = 2^-24, gamma(k) = k u / (1 - k u), no measured quantity enters):
    forward    |y - y64| <= |y64| gamma(C + 4): the C products and C - 1 additions of the sum of squares in any order (relative gamma(C);
               the square root halves it and adds u), the reciprocal (u) and the product (u) stay below C/2 + 3 roundings.
               |inv - inv64| <= inv64 gamma(C + 3), the same without the last product.
    backward   with ey = gamma(C + 4) the relative error of y, ei = gamma(C + 3) that of inv, A = sum_c |y_c g_c|, d = y . g:
               the dot product of the rounded y in any order:            |d' - d| <= A ((1 + ey)(1 + gamma(C)) - 1) =: ed
               the product y' d' rounded:                                |y||d| ((1 + ey)(1 + u) - 1) + |y| ed (1 + ey)(1 + u)
               the difference rounded, then scaled by inv' and rounded:  relative (1 + u)^2 (1 + ei) - 1 on everything
               |gx - gx64| <= inv64 (1 + er) (|y||d| ((1 + ey)(1 + u) - 1) + |y| ed (1 + ey)(1 + u)) + |gx64| er,   er = (1 + u)^2 (1 + ei) - 1
               clamp branch: one correctly rounded division, |gx - gx64| <= |gx64| u; the bound takes gamma(2).
The bounds need the squares and products to stay clear of underflow: every case keeps |x| of a row that is not clamped above 1e-12 and
|g| above 1e-3, and the tests assert that no square underflows and no reference value is subnormal in float32.

Branch at the threshold.  The kernels tell the branches apart by inv == 1 / eps, which a norm one rounding above eps satisfies as well;
a norm that close to eps is within the rounding of the norm itself.  No case puts a norm within a factor 1 +- 2^-10 of eps (asserted).

Cases.  Every row of a matrix has its own scale (SCALES cycles 1, 1e-8, 1e3, 1e-3, 30): a normalisation that mixes rows up, or applies eps
to the squared norm (rows of norm 1e-8 .. 1e-6 then come out wrong), shows.  `grid`: every M of MS at every C of CS.  `special`: rows with
exactly known results between random rows -- see SPECIAL_ROWS.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
EPS = float(np.float32(1e-12))
MS = (1, 3, 255, 257)
CS = (1, 3, 6, 7, 63, 64, 65, 256, 300)         # rows below, at and past a wave, several strides; 6 adds the residue 2 mod 4
SCALES = (1.0, 1e-8, 1e3, 1e-3, 30.0)
# row -> kind, in a matrix of 12 rows; every other row is random
SPECIAL_ROWS = {1: "zero", 3: "below_eps", 5: "nan", 7: "inf", 9: "overflow"}
SPECIAL_M = 12
SPECIAL_CS = (7, 64, 300)
GROUPS = ("grid", "special")


def gamma(k: float) -> float:
    return k * U / (1.0 - k * U)


@dataclass(frozen=True)
class Case:
    group: str
    m: int
    c: int

    @property
    def id(self):
        return f"{self.group}-{self.m}x{self.c}"


GRID = tuple(Case("grid", m, c) for m in MS for c in CS)
SPECIAL = tuple(Case("special", SPECIAL_M, c) for c in SPECIAL_CS)
CASES = GRID + SPECIAL


def _away_from_zero(a):
    """Random normals pushed out of (-1e-3, 1e-3): no live product comes near underflow after the row scale."""
    return np.where(np.abs(a) < 1e-3, np.where(a < 0, -1e-3, 1e-3), a)


@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    """(x, g) float32 [M, C], read-only."""
    rs = np.random.RandomState(7000 + 31 * case.m + case.c + (100000 if case.group == "special" else 0))
    scale = np.array([SCALES[i % len(SCALES)] for i in range(case.m)])[:, None]
    x = (_away_from_zero(rs.randn(case.m, case.c)) * scale).astype(np.float32)
    g = _away_from_zero(rs.randn(case.m, case.c)).astype(np.float32)
    if case.group == "special":
        for row, kind in SPECIAL_ROWS.items():
            col = (3 * row) % case.c
            if kind == "zero":
                x[row] = 0.0
            elif kind == "below_eps":
                x[row] = (_away_from_zero(rs.randn(case.c)) * 1e-15).astype(np.float32)       # norm about 1e-15 sqrt(C) < 1e-13
            elif kind == "nan":
                x[row, col] = np.nan
            elif kind == "inf":
                x[row, col] = np.inf
            elif kind == "overflow":
                x[row] = 1e20
    x.setflags(write=False)
    g.setflags(write=False)
    return x, g


def live_rows(case: Case) -> np.ndarray:
    """bool [M]: rows the bounds apply to (every row but nan / inf / overflow, whose results are stated exactly)."""
    live = np.ones(case.m, dtype=bool)
    if case.group == "special":
        for row, kind in SPECIAL_ROWS.items():
            if kind in ("nan", "inf", "overflow"):
                live[row] = False
    return live


@dataclass
class Result:
    y: np.ndarray
    inv: np.ndarray
    gx: np.ndarray


def reference(x, g, eps=EPS):
    """float64: (Result, clamped rows, Result of bounds)."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    c = x.shape[1]
    with np.errstate(all="ignore"):
        n = np.sqrt((x * x).sum(1))
        clamped = n < eps
        t = np.where(clamped, eps, n)[:, None]
        y, inv = x / t, 1.0 / t[:, 0]
        d = (y * g).sum(1)[:, None]
        a = np.abs(y * g).sum(1)[:, None]
        gx = np.where(clamped[:, None], g / eps, (g - y * d) / t)
        ey, ei = gamma(c + 4), gamma(c + 3)
        ed = a * ((1 + ey) * (1 + gamma(c)) - 1)
        er = (1 + U) ** 2 * (1 + ei) - 1
        prod = np.abs(y) * np.abs(d) * ((1 + ey) * (1 + U) - 1) + np.abs(y) * ed * (1 + ey) * (1 + U)
        b_gx = np.where(clamped[:, None], np.abs(gx) * gamma(2), (1 + er) * prod / t + np.abs(gx) * er)
    return Result(y, inv, gx), clamped, Result(np.abs(y) * ey, np.abs(inv) * ei, b_gx)


@functools.lru_cache(maxsize=None)
def expectation(case: Case):
    return reference(*inputs(case))


def restate32(x, g, eps=EPS, wrong: str | None = None) -> Result:
    """The kernels' formulas in NumPy float32, every operation rounded once (NumPy's own summation order).  `wrong`: one thing wrong --
    no_sqrt (the norm without the square root), no_projection (the backward pass without y (y . g)), eps_on_squared (max(ss, eps) under
    the root)."""
    f = np.float32
    x, g, eps = np.asarray(x, dtype=f), np.asarray(g, dtype=f), f(eps)
    with np.errstate(all="ignore"):
        ss = (x * x).sum(1, dtype=f)
        if wrong == "eps_on_squared":
            n = np.sqrt(np.where(ss < eps, eps, ss))
        else:
            n = ss if wrong == "no_sqrt" else np.sqrt(ss)
        t = np.where(n < eps, eps, n)                      # a NaN norm stays NaN
        inv = f(1) / t
        y = x * inv[:, None]
        d = (y * g).sum(1, dtype=f)[:, None]
        proj = g if wrong == "no_projection" else g - y * d
        gx = np.where((inv == f(1) / eps)[:, None], g / eps, inv[:, None] * proj)
    assert y.dtype == f and inv.dtype == f and gx.dtype == f
    return Result(y, inv, gx)


WRONG = ("no_sqrt", "no_projection", "eps_on_squared")


def violations(case: Case, got: Result) -> dict:
    """name -> number of elements of the live rows outside the bound (non-finite counts)."""
    ref, _, bound = expectation(case)
    live = live_rows(case)
    out = {}
    for name in ("y", "inv", "gx"):
        a, r, b = (np.asarray(getattr(t, name), dtype=np.float64)[live] for t in (got, ref, bound))
        with np.errstate(invalid="ignore"):
            out[name] = int((~(np.abs(a - r) <= b)).sum())
    return out


def worst_ratio(case: Case, got: Result) -> float:
    """max |got - ref| / bound over the live rows (0 / 0 counts as 0): printed before the assertion."""
    ref, _, bound = expectation(case)
    live = live_rows(case)
    w = 0.0
    for name in ("y", "inv", "gx"):
        a, r, b = (np.asarray(getattr(t, name), dtype=np.float64)[live] for t in (got, ref, bound))
        e = np.abs(a - r)
        with np.errstate(all="ignore"):
            q = np.where(e == 0, 0.0, e / b)
        w = max(w, float(np.nanmax(q)) if q.size else 0.0)
    return w


def special_expectation(case: Case) -> dict:
    """row -> Result of exactly known float32 rows (value comparison; NaN where the rule gives NaN):
    zero       y = 0, inv = 1 / eps, gx = g / eps
    below_eps  y = x * (1 / eps) (one product), inv = 1 / eps, gx = g / eps
    nan        y, inv, gx all NaN
    inf        norm = inf, inv = 0: y = x * 0 -- zero, NaN at the inf; gx all NaN (the dot product holds the NaN)
    overflow   the float32 sum of squares is inf, inv = 0: y = 0 and gx = 0 -- torch's own float32 result (test_l2norm_cpu.py)"""
    assert case.group == "special"
    f = np.float32
    x, g = inputs(case)
    eps, nan = f(EPS), np.full(case.c, np.nan, dtype=f)
    inv_eps = f(1) / eps
    out = {}
    for row, kind in SPECIAL_ROWS.items():
        with np.errstate(all="ignore"):
            if kind == "zero":
                out[row] = Result(np.zeros(case.c, dtype=f), inv_eps, g[row] / eps)
            elif kind == "below_eps":
                out[row] = Result(x[row] * inv_eps, inv_eps, g[row] / eps)
            elif kind == "nan":
                out[row] = Result(nan, f(np.nan), nan)
            elif kind == "inf":
                out[row] = Result(x[row] * f(0), f(0), nan)
            elif kind == "overflow":
                out[row] = Result(np.zeros(case.c, dtype=f), f(0), np.zeros(case.c, dtype=f))
    return out


def same_values(a, b) -> bool:
    """Equal as values, NaN equal to NaN (the sign of a zero is not compared)."""
    return bool(np.array_equal(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32), equal_nan=True))
