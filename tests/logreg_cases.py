"""Cases, float64 restatements and error bounds for the logistic-regression kernels (graphpope_amd/csrc/logreg.hip) and
``graphpope_amd.logreg``.  Imports without a GPU; tests/test_logreg_cpu.py checks the restatement and the bounds themselves,
tests/test_logreg_gpu.py holds the device to them.

The restatement
---------------
:func:`restate` is scikit-learn's ``LinearModelLoss.loss_gradient`` (unweighted) written out in NumPy for a dtype: raw = z W^T + b;
more than two classes ``HalfMultinomialLoss`` (softmax around the row maximum), two classes ``HalfBinomialLoss`` in the four branches
of ``closs_grad_half_binomial``; loss = mean row loss + l2/2 |W|^2; grad_W = (P - Y)^T z / m + l2 W; grad_b = column means of
P - Y.  ``w`` and ``grad`` are in scikit-learn's ``ravel(order="F")`` layout: (class c, column j) at ``j * R + c``.  Evaluated in
``np.longdouble`` (u = 2^-64) it is the reference the bounds below are measured against.

The bounds (:func:`bounds`): derived, not tuned
-----------------------------------------------
u = 2^-53, gamma(k) = k u / (1 - k u).  K = 2: library exp / log / log1p are taken to be within 2 ulp (OCML documents 1 ulp for the
float64 forms, glibc stays below 1).  All magnitudes are taken from the longdouble evaluation; ``|.|`` is element-wise.

1. raw.  A float64 dot product of length d + 1 (d products and the intercept), in any order, fused or not:
   |d raw_ic| <= e_ic = gamma(d + 1) (sum_j |z_ij| |W_cj| + |b_c|);  E_i = max_c e_ic.
2. residual.  softmax is p_c(delta) = p_c exp(delta_c) / S, S = sum_k p_k exp(delta_k).  With |delta_k| <= E:
   p_c(delta) - p_c = p_c ((1 - p_c) exp(delta_c) - sum_{k != c} p_k exp(delta_k)) / S, whose numerator is at most
   (1 - p_c)(exp(E) - exp(-E)) in magnitude, and S >= exp(-E):  |d p_c| <= 2 p_c (1 - p_c) sinh(E) exp(E).  (The sigmoid is the
   two-class softmax of (0, raw), so the same holds for it.)  Evaluating it adds roundings: raw_c - max (an absolute u |raw_c - max|
   in the exponent: a relative expm1 of it on p_c), exp (K u), the sum of R positive terms (gamma(R - 1)), the quotient (u) and
   the subtraction of Y (u |r_c|); the binomial branches have no more operations than that.  With c_r = R + 2 K + 4:
   er_ic = 2 p_ic (1 - p_ic) sinh(E_i) exp(E_i) + p_ic expm1(2 u |raw_ic - max_i|) + c_r u (p_ic + |r_ic|).
3. row loss.  logsumexp is 1-Lipschitz in the max norm and raw_y moves by at most e_iy: E_i + e_iy; the evaluation adds the
   relative error of the sum and K u on the logarithm, (R + 3 K + 2) u (1 + |log S|), and three roundings of additions,
   2 u (|max_i| + |raw_iy| + |loss_i|).  The binomial row loss has slope sigmoid - y in [-1, 1] and fewer operations, so the same
   expression with raw_iy = y_i raw_i and S = 1 covers it.
4. sums.  A float64 sum of m products r_ic z_ij in ANY order, fused or not: gamma(m + 1) sum_i |r_ic| |z_ij|, plus what the
   residuals carry in, (1 + gamma(m + 1)) sum_i er_ic |z_ij|; both / m.  The division, the product l2 w and the last addition:
   3 u (sum_i |r_ic| |z_ij| / m + |l2 w|).  The intercept's column has z = 1.  The loss likewise from the row losses, and
   gamma(R d + 2) on l2/2 |W|^2.

Nothing here is taken from what the device returns.  tests/test_logreg_cpu.py asserts that the gradient bound stays below
1e-10 max|grad| on every case: float32 accumulation (u = 2^-24) misses that by six orders of magnitude.
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -53
K_ULP = 2.0


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def blobs(n, d, C, sep, seed):
    """(X float32 [n, d], y int64 [n]): C Gaussian blobs, centres ``sep`` apart per coordinate.  The first n // 2 rows train."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((C, d)) * sep
    y = rng.integers(0, C, n)
    X = np.float32(mu[y] + rng.standard_normal((n, d)))
    return X, y


# (n, d, C, sep, seed, max_iter); scikit-learn 1.7.2 takes 18, 11, 15, 19, 6, 5 and 23 iterations on the float64 copy
FIT_CASES = [
    (600, 128, 7, 0.35, 0, 150),
    (600, 128, 3, 0.35, 1, 150),
    (600, 128, 2, 0.35, 2, 150),
    (300, 33, 5, 0.5, 3, 150),
    (1300, 130, 64, 0.6, 5, 150),
    (600, 128, 7, 0.35, 0, 5),             # stops at the iteration cap and warns
    (4000, 128, 7, 0.2, 6, 150),
]
CAPPED = (600, 128, 7, 0.35, 0, 5)
MARGIN = 1e-6                              # a test row whose scikit-learn top-2 margin is below this may be predicted either way ...
EXCUSED = 0.01                             # ... up to this fraction of a case's test rows (on these inputs: none, smallest margin 1.3e-4)
COEF_CEILING = 1e-9


def fit_split(case):
    """(X_train, y_train, X_test, y_test) of a fit case."""
    n, d, C, sep, seed, _ = case
    X, y = blobs(n, d, C, sep, seed)
    h = n // 2
    return X[:h], y[:h], X[h:], y[h:]


@functools.lru_cache(maxsize=None)
def sklearn_fit(case):
    """scikit-learn on the float64 copy of a fit case, computed once: dict(classes, coef, intercept, n_iter, pred, score, margin)."""
    import warnings
    from sklearn.linear_model import LogisticRegression
    Xtr, ytr, Xte, yte = fit_split(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = LogisticRegression(solver="lbfgs", max_iter=case[5]).fit(Xtr.astype(np.float64), ytr)
    dec = clf.decision_function(Xte.astype(np.float64))
    if dec.ndim == 1:
        margin = np.abs(dec)
    else:
        top = np.sort(dec, axis=1)
        margin = top[:, -1] - top[:, -2]
    return dict(classes=clf.classes_, coef=clf.coef_, intercept=clf.intercept_, n_iter=int(clf.n_iter_[0]),
                pred=clf.predict(Xte.astype(np.float64)), score=clf.score(Xte.astype(np.float64), yte), margin=margin)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def unpack(w, R, d, fit_intercept, dtype=np.float64):
    table = np.asarray(w, dtype=dtype).reshape((R, -1), order="F")
    return table[:, :d], (table[:, d] if fit_intercept else np.zeros(R, dtype=dtype))


def raw_scores(z, w, classes, fit_intercept, dtype=np.float64):
    R = 1 if classes == 2 else classes
    W, b = unpack(w, R, z.shape[1], fit_intercept, dtype)
    return z.astype(dtype) @ W.T + b


def restate(z, y, w, classes, fit_intercept, l2, dtype=np.float64, order=None):
    """dict(loss, grad [R (d + fit_intercept)], raw [m, R], p [m, R], r [m, R], row_loss [m]) in ``dtype``.  ``order``: a permutation of
    the rows to evaluate in (the result is the same function of the inputs; only the summation order moves)."""
    if order is not None:
        z, y = z[order], y[order]
    m, d = z.shape
    R = 1 if classes == 2 else classes
    Z = z.astype(dtype)
    W, b = unpack(w, R, d, fit_intercept, dtype)
    raw = Z @ W.T + b
    one = dtype(1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if R == 1:
            x, yt = raw[:, 0], (y == 1).astype(dtype)
            row_loss, g = np.empty(m, dtype), np.empty(m, dtype)
            b1, b2, b3 = x <= -37, (x > -37) & (x <= -2), (x > -2) & (x <= 18)
            b4 = ~(b1 | b2 | b3)                                               # a NaN lands here, as in the C code's else
            t = np.exp(x[b1]); row_loss[b1] = t - yt[b1] * x[b1]; g[b1] = t - yt[b1]
            t = np.exp(x[b2]); row_loss[b2] = np.log1p(t) - yt[b2] * x[b2]; g[b2] = ((one - yt[b2]) * t - yt[b2]) / (one + t)
            t = np.exp(-x[b3]); row_loss[b3] = np.log1p(t) + (one - yt[b3]) * x[b3]; g[b3] = ((one - yt[b3]) - yt[b3] * t) / (one + t)
            t = np.exp(-x[b4]); row_loss[b4] = t + (one - yt[b4]) * x[b4]; g[b4] = ((one - yt[b4]) - yt[b4] * t) / (one + t)
            r = g[:, None]
            p = r + yt[:, None]                                                 # sigmoid(raw)
        else:
            mx = raw.max(axis=1)
            e = np.exp(raw - mx[:, None])
            s = e.sum(axis=1)
            row_loss = np.log(s) + mx - raw[np.arange(m), y]
            p = e / s[:, None]
            r = p.copy()
            r[np.arange(m), y] -= one
        grad_w = r.T @ Z / dtype(m) + dtype(l2) * W
        grad_b = r.sum(axis=0) / dtype(m)
        loss = row_loss.sum() / dtype(m) + dtype(0.5) * dtype(l2) * (W * W).sum()
    table = np.concatenate([grad_w, grad_b[:, None]], axis=1) if fit_intercept else grad_w
    return dict(loss=loss, grad=table.ravel(order="F"), raw=raw, p=p, r=r, row_loss=row_loss)


def predict_rule(raw):
    """np.argmax's rule (the first maximum) for more than one column, raw > 0 for one."""
    return (raw[:, 0] > 0).astype(np.int32) if raw.shape[1] == 1 else np.argmax(raw, axis=1).astype(np.int32)


def bounds(z, y, w, classes, fit_intercept, l2, ref):
    """(loss bound, gradient bound per element) of one float64 evaluation against the exact value: the derivation in the module's
    docstring, evaluated in float64 on the magnitudes of ``ref`` = ``restate(..., dtype=np.longdouble)``."""
    m, d = z.shape
    R = 1 if classes == 2 else classes
    A = np.abs(z.astype(np.float64))
    W, b = unpack(w, R, d, fit_intercept)
    raw, p, r, row_loss = (np.asarray(ref[k], dtype=np.float64) for k in ("raw", "p", "r", "row_loss"))
    e = gamma(d + 1) * (A @ np.abs(W).T + np.abs(b))                           # 1.
    E = e.max(axis=1)
    if R == 1:
        mx = np.maximum(raw[:, 0], 0.0)
        spread = np.abs(raw[:, 0])                                              # the exponent of the branch taken is +-raw
        raw_y, log_s = (y == 1) * raw[:, 0], np.zeros(m)
        e_y = e[:, 0]
    else:
        mx = raw.max(axis=1)
        spread = np.abs(raw - mx[:, None])
        raw_y = raw[np.arange(m), y]
        log_s = np.abs(np.log(np.exp(raw - mx[:, None]).sum(axis=1)))
        e_y = e[np.arange(m), y]
    spread = spread.reshape(m, R)
    c_r = R + 2 * K_ULP + 4
    er = (2 * p * (1 - p) * (np.sinh(E) * np.exp(E))[:, None] + p * np.expm1(2 * U * spread) + c_r * U * (p + np.abs(r)))   # 2.
    el = E + e_y + (R + 3 * K_ULP + 2) * U * (1 + log_s) + 2 * U * (np.abs(mx) + np.abs(raw_y) + np.abs(row_loss))         # 3.
    A1 = np.concatenate([A, np.ones((m, 1))], axis=1) if fit_intercept else A    # 4.
    mass = np.abs(r).T @ A1 / m
    pen = np.concatenate([np.abs(l2 * W), np.zeros((R, 1))], axis=1) if fit_intercept else np.abs(l2 * W)
    g = (1 + gamma(m + 1)) * (er.T @ A1) / m + gamma(m + 1) * mass + 3 * U * (mass + pen)
    wsq = 0.5 * l2 * (W * W).sum()
    mean_abs = np.abs(row_loss).sum() / m
    lb = (1 + gamma(m)) * el.sum() / m + gamma(m) * mean_abs + gamma(R * d + 2) * wsq + 3 * U * (mean_abs + wsq)
    return float(lb), g.ravel(order="F")


# ---- objective cases ----------------------------------------------------------------------------------------------------------------
SLICE_DEFAULT = 256          # pope_logreg_slice_rows() as the cases were written; the GPU test reads the query and re-derives `ragged`
W_MODES = ("zero", "normal", "big")
BIG_RAW = 800.0              # exp overflows from 709.8


def ragged_rows(slice_rows):
    """At least three row slices, the last one ragged."""
    return 2 * slice_rows + 37


def objective_cases(slice_rows=SLICE_DEFAULT):
    """dicts(id, m, d, classes, pad, icpt, ids, w, seed, nan).  ``pad``: ldz - d; ``ids``: None, or the size N of the table rows are
    selected from (descending, with repeats)."""
    out = []

    def add(m, d, classes, w, pad=0, icpt=True, ids=None, nan=False):
        out.append(dict(id=f"m{m}-d{d}-c{classes}-{w}-pad{pad}-{'b' if icpt else 'nob'}" + (f"-ids{ids}" if ids else "") + ("-nan" if nan else ""),
                        m=m, d=d, classes=classes, pad=pad, icpt=icpt, ids=ids, w=w, seed=len(out), nan=nan))

    for n, d, C in sorted({c[:3] for c in FIT_CASES}):                          # the fit shapes (their training halves)
        for w in W_MODES:
            add(n // 2, d, C, w)
    for m in (1, 63, 64, 65, 257, ragged_rows(slice_rows)):
        add(m, 33, 3, "normal")
        add(m, 33, 2, "big")
    for d in (1, 3, 33, 128, 130):
        for w in ("normal", "big"):
            add(65, d, 7, w, pad=5)
    for classes in (2, 3, 7, 64):
        for icpt in (True, False):
            for w in W_MODES:
                add(257, 33, classes, w, pad=3, icpt=icpt)
    for classes in (2, 7):
        add(200, 33, classes, "normal", pad=2, ids=300)
        add(ragged_rows(slice_rows), 33, classes, "big", ids=300)
    add(70, 33, 3, "normal", nan=True)
    add(70, 33, 2, "normal", nan=True)
    return out


NAN_ROW, NAN_COL = 5, 2


@functools.lru_cache(maxsize=None)
def _objective_inputs(m, d, classes, pad, icpt, ids, w_mode, seed, nan):
    rng = np.random.default_rng(1000 + seed)
    n_table = ids or m
    table = np.float32(rng.standard_normal((n_table, d + pad)))                  # the kernel sees columns [0, d) of rows of stride d + pad
    if ids:
        sel = np.concatenate([np.arange(n_table - 1, -1, -3), rng.integers(0, n_table, m)])[:m].astype(np.int64)
        sel[1] = sel[0]                                                          # a repeat next to its twin, too
    else:
        sel = None
    if nan:
        table[NAN_ROW, NAN_COL] = np.nan
    z = table[:, :d] if sel is None else table[sel, :d]
    y = rng.integers(0, classes, m)
    R = 1 if classes == 2 else classes
    cols = d + (1 if icpt else 0)
    if w_mode == "zero":
        w = np.zeros(R * cols)
    else:
        w = rng.standard_normal(R * cols)
        if w_mode == "big":                                                      # |raw| reaches BIG_RAW, in both signs
            raw = raw_scores(np.nan_to_num(z), w, classes, icpt)
            w *= BIG_RAW / np.abs(raw).max()
    l2 = 1.0 / m
    for a in (table, y, w):
        a.setflags(write=False)
    return table, sel, z, y, w, l2


def objective_inputs(case):
    """(table float32 [N, d + pad], ids int64 [m] or None, z = the selected rows' first d columns, y, w, l2).  Read-only, shared."""
    return _objective_inputs(case["m"], case["d"], case["classes"], case["pad"], case["icpt"], case["ids"], case["w"], case["seed"], case["nan"])


@functools.lru_cache(maxsize=None)
def _reference(m, d, classes, pad, icpt, ids, w_mode, seed, nan):
    _, _, z, y, w, l2 = _objective_inputs(m, d, classes, pad, icpt, ids, w_mode, seed, nan)
    ref = restate(z, y, w, classes, icpt, l2, dtype=np.longdouble)
    lb, gb = (None, None) if nan else bounds(z, y, w, classes, icpt, l2, ref)
    return ref, lb, gb


def reference(case):
    """(longdouble evaluation, loss bound, gradient bounds) of a case, computed once and shared."""
    return _reference(case["m"], case["d"], case["classes"], case["pad"], case["icpt"], case["ids"], case["w"], case["seed"], case["nan"])


# ---- the fit, restated --------------------------------------------------------------------------------------------------------------
def fit_restated(X, y, max_iter, C=1.0, fit_intercept=True, tol=1e-4):
    """scikit-learn's lbfgs fit with :func:`restate` as the callable: dict(classes, coef, intercept, n_iter, w, status)."""
    import scipy.optimize
    classes = np.unique(y)
    enc = np.searchsorted(classes, y)
    n_cls = len(classes)
    R = 1 if n_cls == 2 else n_cls
    m, d = X.shape
    l2 = 1.0 / (C * m)

    def fun(w):
        out = restate(X, enc, w, n_cls, fit_intercept, l2)
        return float(out["loss"]), out["grad"]

    res = scipy.optimize.minimize(fun, np.zeros(R * (d + (1 if fit_intercept else 0))), method="L-BFGS-B", jac=True,
                                  options={"maxiter": max_iter, "maxls": 50, "gtol": tol, "ftol": 64 * np.finfo(float).eps})
    W, b = unpack(res.x, R, d, fit_intercept)
    return dict(classes=classes, coef=W, intercept=b, n_iter=min(int(res.nit), max_iter), w=res.x, status=res.status)


# ---- the planted-partition graph of the end-to-end test --------------------------------------------------------------------------------
def planted_partition(communities=4, size=64, p_in=0.3, p_out=0.005, seed=0):
    """(edge_index int64 [2, E] symmetric, labels int64 [n])."""
    rng = np.random.default_rng(seed)
    n = communities * size
    labels = np.repeat(np.arange(communities), size)
    prob = np.where(labels[:, None] == labels[None, :], p_in, p_out)
    upper = np.triu(rng.random((n, n)) < prob, 1)
    src, dst = np.nonzero(upper | upper.T)
    return np.stack([src, dst]).astype(np.int64), labels
