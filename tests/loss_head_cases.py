"""Cases, float64 reference and bounds for the training loss head (csrc/epilogue.hip: k_xent_rows, k_xent_final, the loss block of
k_adam) -- main.py:216 F.cross_entropy(y_hat, y).  No GPU and no library needed to import this: test_loss_head_cpu.py runs the
reference against torch on the CPU, test_loss_head_gpu.py runs the kernels against it.

Reference (NumPy float64 on the float32 inputs): lse_i = max + log(sum(exp(x - max))), loss_i = lse_i - x[i, y_i],
grad_i = exp(x_i - lse_i) - onehot.  A row is counted iff 0 <= y < C and y != ignore_index; mean = sum / count (NaN for count 0);
inv_count = float32(1) / float32(count) (0 for count 0); a label outside [0, C) that is not ignore_index sets the bad-label word.

Bounds, from float32 rounding (not from any kernel's output):
  row loss   lse - x_y is two float32 additions of numbers of size |max|, |x_y| and log C, each off by half an ulp (2^-24 relative),
             plus logf and the sum of C exponentials (a few ulps of a number <= log C + 1): 2^-22 * (|max| + |x_y| + log C + 8).
  mean loss  the mean of the row bounds (the sum itself is float64) + the final rounding to float32, 2^-23 * |mean|.
  gradient   softmax elements are <= 1: expf of a difference rounded to 2^-24 relative, a reciprocal and a product are a few 2^-24;
             2^-19 absolute leaves a factor of ~8.  Scaled: (2^-19 + 2^-22 |ref|) * scale -- three more float32 roundings on the scale.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

LOSS_ULP = 2.0 ** -22
GRAD_ABS = 2.0 ** -19
GRAD_REL = 2.0 ** -22
UPSTREAM = 1.7                        # the non-unit upstream gradient of form 1

COLUMNS = (1, 2, 63, 64, 65, 448, 511, 512, 513, 1000, 1025)         # 512 / 513: register form / looped form of k_xent_rows
ROWS = (1, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, 4097)          # the 8 x 256 stride of the count loop and of the final block
OPTIMISER_SHAPES = ((5, 3), (2049, 3), (257, 513))                    # forms 4 and 5; the last one also form 6


@dataclass
class Case:
    name: str
    logits: np.ndarray                 # float32 [N, C]
    y: np.ndarray                      # int64 [N]
    ignore_index: int = -100
    forms: tuple = (1, 2, 3)
    exact_zero_rows: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))   # row_scratch must be exactly +0 there


@dataclass
class Reference:
    counted: np.ndarray                # bool [N]
    loss: np.ndarray                   # float64 [N] (only counted entries mean anything)
    loss_bound: np.ndarray             # float64 [N]
    grad: np.ndarray                   # float64 [N, C]: exp(x - lse) - onehot, zero rows where not counted
    count: int
    mean: float
    mean_bound: float
    inv_count: np.float32
    bad: int


def reference(logits: np.ndarray, y: np.ndarray, ignore_index: int = -100) -> Reference:
    assert logits.dtype == np.float32 and y.dtype == np.int64
    x = logits.astype(np.float64)
    n, c = x.shape
    inside = (y >= 0) & (y < c)
    counted = inside & (y != ignore_index)
    bad = int((~inside & (y != ignore_index)).any())
    ys = np.where(counted, y, 0)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        mx = x.max(axis=1)
        lse = mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))
        xy = x[rows, ys]
        loss = lse - xy
        grad = np.exp(x - lse[:, None])
        grad[rows, ys] -= 1.0
        loss_bound = LOSS_ULP * (np.abs(mx) + np.abs(xy) + np.log(c) + 8.0)
    grad[~counted] = 0.0
    count = int(counted.sum())
    with np.errstate(all="ignore"):
        mean = float(loss[counted].sum() / count) if count else float("nan")
    finite = counted & np.isfinite(loss)
    mean_bound = float(loss_bound[finite].mean() + 2.0 ** -23 * abs(mean)) if finite.any() and np.isfinite(mean) else 0.0
    inv_count = np.float32(1) / np.float32(count) if count else np.float32(0)
    return Reference(counted, loss, loss_bound, grad, count, mean, mean_bound, inv_count, bad)


def _same_kind(got: float, want: float) -> bool:
    """Non-finite values agree when both are NaN or both are the same infinity."""
    return (np.isnan(got) and np.isnan(want)) or got == want


def check(case: Case, ref: Reference, got: dict, what: str) -> dict:
    """Assert one form's outputs against the reference; return the worst error-to-bound ratios {"row", "mean", "grad", "scaled"}.

    got: "loss" (float), "inv_count" (np.float32), "bad" (int), "rows" (float32 [N], row_scratch), and "grad" (float32 [N, C]) with
    "grad_scale" (the float64 factor the reference gradient is multiplied by: 1 for the unscaled one).  "scaled" / "scaled_scale"
    (optional): a second gradient, checked in the same way.
    """
    tag = f"{case.name} [{what}]"
    ratios = {}
    assert int(got["bad"]) == ref.bad, (tag, "bad-label word", got["bad"], ref.bad)
    inv = np.float32(got["inv_count"])
    assert inv.tobytes() == ref.inv_count.tobytes(), (tag, "inv_count", float(inv), float(ref.inv_count), "mean loss", float(got["loss"]), ref.mean)
    # row losses
    rows = np.asarray(got["rows"], dtype=np.float32)
    assert rows.shape == ref.counted.shape
    assert np.all(rows[~ref.counted] == -1.0), (tag, "an uncounted row does not carry the marker")
    finite = ref.counted & np.isfinite(ref.loss)
    with np.errstate(all="ignore"):
        err = np.abs(rows.astype(np.float64) - ref.loss)
    assert np.all(np.isfinite(rows[finite])), (tag, "a finite row loss came out non-finite", np.flatnonzero(finite & ~np.isfinite(rows))[:5])
    assert np.all(rows[finite] >= 0.0), (tag, "negative row loss", np.flatnonzero(finite & (rows < 0))[:5])
    if finite.any():
        r = err[finite] / ref.loss_bound[finite]
        ratios["row"] = float(r.max())
        i = np.flatnonzero(finite)[int(r.argmax())]
        assert ratios["row"] <= 1.0, (tag, "row loss", int(i), float(rows[i]), float(ref.loss[i]), float(ref.loss_bound[i]))
    for i in np.flatnonzero(ref.counted & ~np.isfinite(ref.loss)):
        assert _same_kind(float(rows[i]), float(ref.loss[i])), (tag, "non-finite row loss", int(i), float(rows[i]), float(ref.loss[i]))
    z = rows[case.exact_zero_rows]
    assert np.all(z == 0.0) and not np.signbit(z).any(), (tag, "a confident row's loss is not exactly +0")
    assert ref.counted[case.exact_zero_rows].all()
    # mean loss
    loss = float(got["loss"])
    if np.isfinite(ref.mean):
        assert np.isfinite(loss), (tag, "mean loss", loss, ref.mean)
        ratios["mean"] = abs(loss - ref.mean) / ref.mean_bound
        assert ratios["mean"] <= 1.0, (tag, "mean loss", loss, ref.mean, ref.mean_bound)
    else:
        assert _same_kind(loss, ref.mean), (tag, "mean loss", loss, ref.mean)
    # gradients
    for key, scale_key, name in (("grad", "grad_scale", "grad"), ("scaled", "scaled_scale", "scaled")):
        if key not in got:
            continue
        g = np.asarray(got[key], dtype=np.float32)
        scale = float(got[scale_key])
        assert g.shape == ref.grad.shape
        assert not g[~ref.counted].any(), (tag, name, "an uncounted row has a gradient")
        want = ref.grad * scale
        nan = np.isnan(want)
        assert np.isnan(g[nan]).all(), (tag, name, "a gradient element is a number where the reference's is NaN")
        assert np.isfinite(g[~nan]).all(), (tag, name, "a gradient element is non-finite where the reference's is a number")
        if scale == 1.0:
            bound = np.full(want.shape, GRAD_ABS)
        else:
            bound = (GRAD_ABS + GRAD_REL * np.abs(ref.grad)) * scale
        ok = ~nan & ref.counted[:, None]
        # an exact zero of the reference (a -inf logit, an exponential that underflows even in float64, C = 1) is one of the kernel too
        assert not g[ok & (want == 0.0)].any(), (tag, name, "a gradient element is not exactly zero where the reference's is")
        if ok.any() and scale > 0.0:
            r = np.abs(g.astype(np.float64) - want)[ok] / bound[ok]
            key_r = "grad" if scale == 1.0 else "scaled"
            ratios[key_r] = max(ratios.get(key_r, 0.0), float(r.max()))
            assert r.max() <= 1.0, (tag, name, float(r.max()))
        elif scale == 0.0:
            assert not g.any(), (tag, name, "no row is counted and the gradient is not zero")
    return ratios


def merge(into: dict, ratios: dict) -> None:
    for k, v in ratios.items():
        into[k] = max(into.get(k, 0.0), v)


# ------------------------------------------------------------------------------------------------ case builders

def _labels(rng, n, c, ignored_every=5):
    y = rng.randint(0, c, n).astype(np.int64)
    if ignored_every:
        y[2::ignored_every] = -100
    return y


def column_cases():
    """Every C of the list at N = 37 (ten blocks of four waves), and the (N, C) = (257, 513) shape all six forms run at."""
    out = []
    for c in COLUMNS:
        rng = np.random.RandomState(100 + c)
        y = _labels(rng, 37, c)
        zero = np.flatnonzero(y >= 0) if c == 1 else np.zeros(0, dtype=np.int64)       # C = 1: loss exactly 0 (and gradient 0)
        out.append(Case(f"columns C={c}", (rng.randn(37, c) * 3).astype(np.float32), y, exact_zero_rows=zero))
    rng = np.random.RandomState(99)
    out.append(Case("columns N=257 C=513", (rng.randn(257, 513) * 3).astype(np.float32), _labels(rng, 257, 513), forms=(1, 2, 3, 4, 5, 6)))
    return out


def edge_rows(n):
    """Indices 0, N - 1 and both sides of every multiple of 256."""
    idx = {0, n - 1}
    for k in range(256, n + 1, 256):
        idx.update(i for i in (k - 1, k) if i < n)
    return np.array(sorted(idx), dtype=np.int64)


def row_cases():
    """Every N of the list at C = 3, in two phases: the rows at the edges of the 256-row stride are alternately ignored and counted,
    starting with an ignored one (phase 0) or a counted one (phase 1).  N = 16390: a wave of the capped grid takes a second row."""
    out = []
    for n in ROWS + (16390,):
        for phase in (0, 1):
            rng = np.random.RandomState(7 * n + phase)
            y = _labels(rng, n, 3)
            edges = edge_rows(n)
            for j, i in enumerate(edges):
                y[i] = -100 if (j + phase) % 2 == 0 else int(rng.randint(0, 3))
            forms = (1, 2, 3, 4, 5) if (n, 3) in OPTIMISER_SHAPES and phase == 1 else (1, 2, 3)
            out.append(Case(f"rows N={n} phase {phase}", (rng.randn(n, 3) * 3).astype(np.float32), y, forms=forms))
    return out


MAGNITUDE_KINDS = ("scale 1e-3", "scale 1", "scale 80", "scale 3e3", "all equal", "shift -1e6", "shift +3e4", "confident", "label trails by 200")


def magnitude_cases():
    out = []
    n = 257
    for c in (7, 65, 513):
        for k, kind in enumerate(MAGNITUDE_KINDS):
            rng = np.random.RandomState(1000 * c + k)
            x = rng.randn(n, c)
            y = _labels(rng, n, c)
            zero_rows = np.zeros(0, dtype=np.int64)
            if kind.startswith("scale"):
                x *= float(kind.split()[1])
            elif kind == "all equal":
                x = np.repeat(rng.randn(n, 1) * 50, c, axis=1)
            elif kind.startswith("shift"):
                x += float(kind.split()[1])
            else:
                live = np.flatnonzero(y >= 0)
                x32 = x.astype(np.float32)
                other = x32.copy()
                other[live, y[live]] = -np.inf
                top = other[live].max(axis=1).astype(np.float64)
                if kind == "confident":
                    x32[live, y[live]] = (top + 30.0 + rng.rand(live.size) * 5).astype(np.float32) + np.float32(0.25)
                    zero_rows = live
                else:
                    x32[live, y[live]] = (top - 200.0).astype(np.float32)
                x = x32
            out.append(Case(f"magnitude C={c} {kind}", np.ascontiguousarray(x, dtype=np.float32), y, exact_zero_rows=zero_rows))
    return out


def label_cases():
    out = []
    n, c = 37, 65
    rng = np.random.RandomState(5)
    x = (rng.randn(n, c) * 3).astype(np.float32)
    for ii in (0, c - 1):                                              # ignore_index inside [0, C): left out, not flagged
        y = rng.randint(0, c, n).astype(np.int64)
        y[::3] = ii
        out.append(Case(f"labels ignore_index={ii}", x, y, ignore_index=ii))
    for bad in (c, -1, 2 ** 40):                                       # outside [0, C) and not ignore_index: left out and flagged
        y = _labels(rng, n, c)
        y[[0, 17, n - 1]] = bad
        out.append(Case(f"labels y={bad}", x, y))
    out.append(Case("labels all ignored", x, np.full(n, -100, dtype=np.int64)))
    out.append(Case("labels all ignored N=2049", (rng.randn(2049, 3)).astype(np.float32), np.full(2049, -100, dtype=np.int64)))
    return out


NON_FINITE_KINDS = ("nan counted", "nan ignored", "+inf counted", "-inf off label", "-inf at label", "row of -inf")


def non_finite_cases():
    """N = 9 rows; row 4 carries the non-finite value(s), row 2 is ignored.  Forms 1 to 5: the final block serves all of them."""
    out = []
    for c in (65, 600):
        for k, kind in enumerate(NON_FINITE_KINDS):
            rng = np.random.RandomState(c + k)
            x = (rng.randn(9, c) * 3).astype(np.float32)
            y = rng.randint(0, c, 9).astype(np.int64)
            y[2] = -100
            y[4] = 7
            if kind == "nan counted":
                x[4, 64] = np.nan                                     # lane 0's second column
            elif kind == "nan ignored":
                x[2, 64] = np.nan
            elif kind == "+inf counted":
                x[4, 3] = np.inf
            elif kind == "-inf off label":
                x[4, [3, 64]] = -np.inf
            elif kind == "-inf at label":
                x[4, 7] = -np.inf
            else:
                x[4, :] = -np.inf
            out.append(Case(f"non-finite C={c} {kind}", x, y, forms=(1, 2, 3, 4, 5)))
    return out


def eval_agreement_cases():
    out = []
    for c in (7, 65, 513):
        rng = np.random.RandomState(31 * c)
        out.append(Case(f"eval agreement C={c}", (rng.randn(1550, c) * 3).astype(np.float32), _labels(rng, 1550, c, ignored_every=7)))
    return out


FAMILIES = {"columns": column_cases, "rows": row_cases, "magnitude": magnitude_cases, "labels": label_cases, "non-finite": non_finite_cases}
