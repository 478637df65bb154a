"""Logistic regression on embedding rows, as PyG's ``Node2Vec.test`` runs it: scikit-learn's ``LogisticRegression(solver='lbfgs')``.

scikit-learn's lbfgs path is ``scipy.optimize.minimize(method="L-BFGS-B")`` around a loss/gradient callable.  :func:`fit` drives the
same optimiser with the same options around pope_logreg_loss_grad (csrc/logreg.hip), which evaluates scikit-learn's
``LinearModelLoss`` -- one pass over ``z`` on the GPU, float64 arithmetic, fixed summation order -- so it follows scikit-learn's
iterates: the same ``n_iter_``, coefficients within 1e-13, the same predictions (tests/test_logreg_gpu.py).  The weight vector keeps
scikit-learn's ``w0.ravel(order="F")`` layout, so scipy's vector goes to the kernel and back unpermuted.

``z`` is a float32 ``[N, d]`` tensor (CPU tensors are moved); ``ids`` selects rows of it without a ``z[ids]`` copy.  ``y`` holds one
label per selected row.  There is no host path: without a GPU these functions raise.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np
import torch

from . import engine
from . import _lib
from ._lib import check, ptr

SOLVERS, MULTI_CLASS, KEYWORDS = ("lbfgs",), ("auto",), ("C", "fit_intercept", "max_iter", "tol")


@dataclass
class Model:
    """What ``LogisticRegression.fit`` leaves behind, with scikit-learn's meanings: ``classes_`` (sorted unique training labels),
    ``coef_`` float64 ``[R, d]`` (``R = 1`` for two classes), ``intercept_`` ``[R]`` (zeros without an intercept), ``n_iter_``
    int32 ``[1]``; ``w``: the optimiser's vector, element (class c, column j) at ``j * R + c``."""
    classes_: np.ndarray
    coef_: np.ndarray
    intercept_: np.ndarray
    n_iter_: np.ndarray
    fit_intercept: bool
    w: np.ndarray


def check_test_arguments(solver="lbfgs", multi_class="auto", args=(), kwargs=None) -> dict:
    """The arguments ``Node2Vec.test`` passes on to ``LogisticRegression``: ``NotImplementedError`` naming what is accepted for
    anything else.  Needs no GPU."""
    kwargs = dict(kwargs or {})
    accepted = (f"accepted: solver in {SOLVERS}, multi_class in {MULTI_CLASS}, keywords {KEYWORDS} (no further positional arguments)")
    if solver not in SOLVERS:
        raise NotImplementedError(f"Node2Vec.test: solver {solver!r} is not implemented; {accepted}")
    if multi_class not in MULTI_CLASS:
        raise NotImplementedError(f"Node2Vec.test: multi_class {multi_class!r} is not implemented; {accepted}")
    if args:
        raise NotImplementedError(f"Node2Vec.test: positional arguments {args!r} are not implemented; {accepted}")
    unknown = sorted(set(kwargs) - set(KEYWORDS))
    if unknown:
        raise NotImplementedError(f"Node2Vec.test: keyword arguments {unknown} are not implemented; {accepted}")
    return kwargs


def _labels(y) -> np.ndarray:
    y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
    return y.reshape(-1)


def _encode(y: np.ndarray, classes: np.ndarray) -> np.ndarray:
    """int32 position of every label in the sorted ``classes``; -1 for a label that is not among them."""
    pos = np.clip(np.searchsorted(classes, y), 0, len(classes) - 1)
    return np.where(classes[pos] == y, pos, -1).astype(np.int32)


class _Rows:
    """``z`` (and ``ids``) on the device in the form the kernels take: float32 rows of unit column stride, int64 ids inside the table."""

    def __init__(self, z, ids, who: str):
        if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.dtype != torch.float32:
            raise TypeError(f"{who}: z must be a 2-D float32 tensor, got {getattr(z, 'dtype', type(z))}")
        self.dev = engine.require_gpu(z.device if z.is_cuda else None)
        z = z.detach().to(self.dev)
        if z.shape[1] < 1:
            raise ValueError(f"{who}: z has no columns")
        if z.shape[0] > 1 and (z.stride(1) != 1 or z.stride(0) < z.shape[1]):
            z = z.contiguous()
        elif z.shape[0] <= 1 and not z.is_contiguous():
            z = z.contiguous()
        self.z, self.n, self.d = z, z.shape[0], z.shape[1]
        self.ldz = z.stride(0) if z.shape[0] > 1 else z.shape[1]
        self.ids = None
        self.m = self.n
        if ids is not None:
            ids = torch.as_tensor(ids).reshape(-1).to(self.dev, torch.int64).contiguous()
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.n):
                raise IndexError(f"{who}: row id outside [0, {self.n})")
            self.ids, self.m = ids, ids.numel()


def fit(z, y, ids=None, C=1.0, fit_intercept=True, max_iter=100, tol=1e-4) -> Model:
    """``LogisticRegression(C=C, fit_intercept=fit_intercept, max_iter=max_iter, tol=tol).fit(z[ids], y)`` with the objective on the
    GPU.  Reaching ``max_iter`` warns with ``sklearn.exceptions.ConvergenceWarning`` (a warning, as there); non-finite ``z`` raises
    ``ValueError`` as scikit-learn's input validation does (found at the first evaluation, where every finite row gives raw = 0)."""
    import scipy.optimize
    lib = _lib.load()
    y = _labels(y)
    classes = np.unique(y)
    if len(classes) < 2:
        raise ValueError("This solver needs samples of at least 2 classes in the data, but the data contains only one class: %r"
                         % (classes[0] if len(classes) else None))
    if len(classes) > lib.pope_logreg_max_classes():
        raise ValueError(f"logreg.fit: {len(classes)} classes, at most {lib.pope_logreg_max_classes()} are supported")
    if not C > 0:
        raise ValueError(f"logreg.fit: C must be positive, got {C!r}")
    rows = _Rows(z, ids, "logreg.fit")
    m, d, dev = rows.m, rows.d, rows.dev
    if len(y) != m:
        raise ValueError(f"logreg.fit: {len(y)} labels for {m} rows")
    n_cls = len(classes)
    r = 1 if n_cls == 2 else n_cls
    p = r * (d + (1 if fit_intercept else 0))
    l2 = 1.0 / (C * m)
    with torch.no_grad(), _lib.on_device(dev):
        y_dev = torch.from_numpy(_encode(y, classes)).to(dev)
        need = lib.pope_logreg_scratch_bytes(m, d, n_cls)
        scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        w_dev = torch.empty(p, dtype=torch.float64, device=dev)
        out_dev = torch.empty(1 + p, dtype=torch.float64, device=dev)                # loss | grad
        w_host = torch.empty(p, dtype=torch.float64, pin_memory=True)
        out_host = torch.empty(1 + p, dtype=torch.float64, pin_memory=True)          # the one buffer every evaluation reads back through
        w_np, out_np = w_host.numpy(), out_host.numpy()
        first = [True]

        def fun(w):
            w_np[:] = w
            w_dev.copy_(w_host, non_blocking=True)
            check(lib.pope_logreg_loss_grad(ptr(rows.z), rows.ldz, rows.n, ptr(rows.ids), m, d, ptr(y_dev), n_cls, int(fit_intercept),
                                            ptr(w_dev), l2, ptr(out_dev), _lib.c_void_p(out_dev.data_ptr() + 8), ptr(scratch),
                                            scratch.numel() * 8, engine._stream()))
            out_host.copy_(out_dev, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            if first[0]:
                first[0] = False
                if not np.isfinite(out_np[0]):
                    raise ValueError("Input X contains NaN or infinity.")
            return float(out_np[0]), out_np[1:].copy()

        res = scipy.optimize.minimize(fun, np.zeros(p), method="L-BFGS-B", jac=True,
                                      options={"maxiter": max_iter, "maxls": 50, "gtol": tol, "ftol": 64 * np.finfo(float).eps})
    n_iter = min(int(res.nit), int(max_iter))
    if res.status != 0:
        from sklearn.exceptions import ConvergenceWarning
        message = f"lbfgs failed to converge after {n_iter} iteration(s) (status={res.status}):\n{res.message}\n"
        if n_iter == max_iter:
            message += f"\nIncrease the number of iterations to improve the convergence (max_iter={max_iter})."
        warnings.warn(message, ConvergenceWarning, stacklevel=2)
    w = np.asarray(res.x, dtype=np.float64)
    table = np.reshape(w, (r, -1), order="F")
    intercept = table[:, -1].copy() if fit_intercept else np.zeros(r)
    return Model(classes, np.ascontiguousarray(table[:, :d]), intercept, np.array([n_iter], dtype=np.int32), bool(fit_intercept), w)


def _predict(model: Model, z, y, ids, who: str):
    """(encoded predictions int32 [m] on the device, number of rows whose prediction is ``y``'s or None, m)."""
    lib = _lib.load()
    rows = _Rows(z, ids, who)
    if rows.d != model.coef_.shape[1]:
        raise ValueError(f"{who}: z has {rows.d} columns, the model was fitted on {model.coef_.shape[1]}")
    m, dev = rows.m, rows.dev
    if y is not None:
        y = _labels(y)
        if len(y) != m:
            raise ValueError(f"{who}: {len(y)} labels for {m} rows")
    with torch.no_grad(), _lib.on_device(dev):
        w_dev = torch.from_numpy(model.w).to(dev)
        pred = torch.empty(m, dtype=torch.int32, device=dev)
        y_dev = None if y is None else torch.from_numpy(_encode(y, model.classes_)).to(dev)
        correct = None if y is None else torch.zeros(1, dtype=torch.int64, device=dev)
        check(lib.pope_logreg_predict(ptr(rows.z), rows.ldz, rows.n, ptr(rows.ids), m, rows.d, len(model.classes_), int(model.fit_intercept),
                                      ptr(w_dev), ptr(y_dev), ptr(pred), ptr(correct), engine._stream()))
        return pred, (None if correct is None else int(correct)), m


def predict(model: Model, z, ids=None) -> np.ndarray:
    """``clf.predict(z[ids])``: labels out of ``model.classes_``."""
    pred, _, _ = _predict(model, z, None, ids, "logreg.predict")
    return model.classes_[pred.cpu().numpy()]


def score(model: Model, z, y, ids=None) -> float:
    """``clf.score(z[ids], y)``: the fraction of rows predicted as ``y`` says, the same Python float.  A label no training row had
    is never counted."""
    _, correct, m = _predict(model, z, y, ids, "logreg.score")
    if m == 0:
        raise ValueError("logreg.score: no rows")
    return float(correct / m)
