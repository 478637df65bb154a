"""``Node2Vec`` with the constructor and the methods of ``torch_geometric.nn.Node2Vec``, on libgraphpope_hip.so.

What /root/reference/generate_node2vec_embedding.py:23-25 builds out of PyG and torch_cluster (neither exists offline):

=============================  =============================================================
PyG Node2Vec                   here
=============================  =============================================================
random_walk (torch_cluster)    pope_n2v_walks: uniform first-order walks over the device CSR (Node2Vec: p = q = 1 only);
                               pope_n2v_walks_biased: second-order (p, q) walks (SecondOrderNode2Vec: any finite p, q > 0)
torch.randint in neg_sample    the same launch: negative rows from the same counter hash
pos_sample / neg_sample        walk rows -> window matrices in PyG's order (pope_n2v_windows)
loss                           pope_n2v_loss_grad, evaluated literally as -log(sigmoid(out) + 1e-15) / -log(1 - sigmoid(out) + 1e-15)
torch.optim.SparseAdam         pope_n2v_sparse_adam: one launch over the N rows, untouched rows and their moments left alone
test                           pope_logreg_loss_grad / pope_logreg_predict under scipy's L-BFGS-B, driven as scikit-learn's
                               LogisticRegression(solver='lbfgs') drives it (logreg.py); test_nodes: the same through row ids
=============================  =============================================================

The random stream is this library's own counter hash, not torch_cluster's: walks are uniform and reproducible in ``seed``, but they are
not the walks PyG would draw.  The initial table IS PyG's: ``torch.nn.Embedding(N, D)`` initialised on the CPU and then moved, a pure
function of the torch CPU seed.  A walk takes ``walk_length`` steps, so a row has ``walk_length + 1`` nodes and
``walk_length + 2 - context_size`` windows (PyG itself takes ``walk_length - 1`` steps).  The gradient is accumulated with float atomic adds, so its last bits -- and after training the last
bits of the table -- may differ between two runs; walks, negatives and the untrained table are bitwise reproducible.

In the library's deterministic mode (``sage.set_deterministic`` / ``with sage.deterministic():`` / ``GRAPHPOPE_DETERMINISTIC=1`` for the
generator) :func:`loss_grad` stores one gradient row per walk position (pope_n2v_position_grads) and sums them per node in a fixed
order, in float64 (pope_n2v_accumulate_det): :meth:`Node2Vec.step`, :meth:`Node2Vec.fit` and :meth:`Node2Vec.loss` are then pure
functions of their inputs, and a seed fixes the trained table to the bit (same binary, same device).
"""
from __future__ import annotations

import math

import torch

from . import engine
from . import _lib
from ._lib import check, ptr
from .sage import is_deterministic

EPS = 1e-15            # PyG's constant inside the two logarithms; the kernel carries the same literal
_MASK64 = (1 << 64) - 1


def _as_rows(t: torch.Tensor, dev) -> torch.Tensor:
    return t.to(dev, torch.int64).contiguous()


def walks(rowptr, col, num_nodes: int, starts, walk_length: int, seed: int, first_row: int = 0, positive: bool = True, negative: bool = True):
    """(pos [B, L + 1] or None, neg [B, L + 1] or None) from ``starts`` [B] in one pope_n2v_walks launch: row i of either kind starts at
    ``starts[i]`` and draws from the counter hash of ``(seed, first_row + i, step, kind)``."""
    lib = _lib.load()
    dev = rowptr.device
    starts = _as_rows(starts, dev)
    b = starts.numel()
    with _lib.on_device(dev):
        pos = torch.empty(b, walk_length + 1, dtype=torch.int64, device=dev) if positive else None
        neg = torch.empty(b, walk_length + 1, dtype=torch.int64, device=dev) if negative else None
        check(lib.pope_n2v_walks(ptr(rowptr), ptr(col), num_nodes, ptr(starts), b, b if negative else 0, walk_length, seed & _MASK64,
                                 first_row, ptr(pos), ptr(neg), engine._stream()))
    return pos, neg


def _check_pq(p, q) -> None:
    """``ValueError`` unless ``p`` and ``q`` are finite and > 0: the condition of pope_n2v_walks_biased, checked without a GPU."""
    for name, v in (("p", p), ("q", q)):
        if not (isinstance(v, (int, float)) and math.isfinite(v) and v > 0):
            raise ValueError(f"node2vec: {name} must be a finite number > 0, got {v!r}")


def walks_biased(rowptr, col, num_nodes: int, starts, walk_length: int, seed: int, p: float, q: float, first_row: int = 0):
    """pos [B, L + 1] int64: second-order (p, q) walks from ``starts`` [B] in one pope_n2v_walks_biased launch.  Every CSR row must be
    ascending (``engine.build_csr_canonical``).  Row i draws from the counter hash of ``(seed, first_row + i, step, try)``;
    ``p = q = 1`` gives :func:`walks`' positive rows bit for bit."""
    _check_pq(p, q)
    lib = _lib.load()
    dev = rowptr.device
    starts = _as_rows(starts, dev)
    b = starts.numel()
    with _lib.on_device(dev):
        pos = torch.empty(b, walk_length + 1, dtype=torch.int64, device=dev)
        check(lib.pope_n2v_walks_biased(ptr(rowptr), ptr(col), num_nodes, ptr(starts), b, walk_length, seed & _MASK64, first_row,
                                        float(p), float(q), ptr(pos), engine._stream()))
    return pos


def windows(rows: torch.Tensor, context_size: int) -> torch.Tensor:
    """[R, len] walk rows -> PyG's window matrix [(len + 1 - C) * R, C]: ``torch.cat([rows[:, j:j + C] for j in ...], 0)``."""
    lib = _lib.load()
    rows = rows.contiguous()
    r, length = rows.shape
    with _lib.on_device(rows.device):
        out = torch.empty((length + 1 - context_size) * r, context_size, dtype=torch.int64, device=rows.device)
        check(lib.pope_n2v_windows(ptr(rows), r, length, context_size, ptr(out), engine._stream()))
    return out


class DetWork:
    """The buffers of the deterministic pair for one device: ``ids`` [M], ``contrib`` [M, D], ``row_loss`` [R] and the index
    ``scratch``, allocated on first use and regrown only when a larger call arrives.  Calls on one stream may share one."""

    def __init__(self):
        self.ids = self.contrib = self.row_loss = self.scratch = None

    def fit(self, r: int, length: int, n: int, d: int, dev):
        """Views for ``r`` rows of ``length`` nodes over an ``[n, d]`` table: (ids, contrib, row_loss, scratch)."""
        m = r * length
        need = _lib.load().pope_n2v_accumulate_det_scratch_bytes(m, n)
        if self.ids is None or self.ids.device != dev or self.ids.numel() < m:
            self.ids = torch.empty(m, dtype=torch.int32, device=dev)
        if self.contrib is None or self.contrib.device != dev or self.contrib.numel() < m * d:
            self.contrib = torch.empty(m * d, dtype=torch.float32, device=dev)
        if self.row_loss is None or self.row_loss.device != dev or self.row_loss.numel() < r:
            self.row_loss = torch.empty(r, dtype=torch.float64, device=dev)
        if self.scratch is None or self.scratch.device != dev or self.scratch.numel() < need:
            self.scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        return self.ids[:m], self.contrib[:m * d].view(m, d), self.row_loss[:r], self.scratch


def position_grads(emb, rows, context_size: int, negative: bool, scale: float, work: DetWork | None = None):
    """(ids int32 [R * len], contrib float32 [R * len, D], row_loss float64 [R]): one gradient row per walk position, stored and not
    added, and the unscaled loss of every row (pope_n2v_position_grads).  ``work``: buffers to write into instead of fresh ones."""
    lib = _lib.load()
    assert emb.is_cuda and emb.dtype == torch.float32 and emb.is_contiguous() and rows.is_contiguous() and rows.dtype == torch.int64
    n, d = emb.shape
    r, length = rows.shape
    with _lib.on_device(emb.device):
        ids, contrib, row_loss, _ = (work or DetWork()).fit(r, length, n, d, emb.device)
        check(lib.pope_n2v_position_grads(ptr(emb), n, d, ptr(rows), r, length, context_size, 1 if negative else 0, scale, ptr(ids),
                                          ptr(contrib), ptr(row_loss), engine._stream()))
    return ids, contrib, row_loss


def accumulate_det(ids, contrib, grad, touched, row_loss, scale: float, loss_acc, scratch=None) -> None:
    """``grad[v] += `` the float64 sum of ``contrib[e]`` over the entries ``ids[e] == v`` in ascending ``e``, rounded once;
    ``touched[v] = 1``; ``loss_acc += scale * sum(row_loss)`` in a fixed order (pope_n2v_accumulate_det).  ``grad`` None: the loss
    part alone; ``row_loss`` None: the gradient part alone."""
    lib = _lib.load()
    with_grad = grad is not None
    m, d = contrib.shape
    assert ids.dtype == torch.int32 and ids.numel() == m and ids.is_contiguous() and contrib.dtype == torch.float32 and contrib.is_contiguous()
    assert not with_grad or (grad.dtype == torch.float32 and grad.is_contiguous() and grad.shape[1] == d and touched.dtype == torch.uint8
                             and touched.numel() == grad.shape[0])
    assert row_loss is None or (row_loss.dtype == torch.float64 and row_loss.is_contiguous() and loss_acc.dtype == torch.float64)
    n = grad.shape[0] if with_grad else 1
    dev = contrib.device
    with _lib.on_device(dev):
        need = lib.pope_n2v_accumulate_det_scratch_bytes(m, n) if with_grad else 0
        if with_grad and (scratch is None or scratch.numel() * scratch.element_size() < need):
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        check(lib.pope_n2v_accumulate_det(ptr(ids), m if with_grad else 0, ptr(contrib), d, n, ptr(grad), ptr(touched), ptr(row_loss),
                                          0 if row_loss is None else row_loss.numel(), scale, ptr(loss_acc), ptr(scratch),
                                          0 if scratch is None else scratch.numel() * scratch.element_size(), engine._stream()))


def loss_grad(emb, rows, context_size: int, negative: bool, scale: float, loss_acc, grad=None, touched=None, work: DetWork | None = None) -> None:
    """``loss_acc += scale * sum of terms``; with ``grad``: ``grad += scale * gradient``, ``touched[v] = 1``.  One pope_n2v_loss_grad
    launch (float atomic adds); in the library's deterministic mode (``sage.is_deterministic()``) :func:`position_grads` and then
    :func:`accumulate_det`, whose result is a pure function of the inputs (``work``: their buffers, else allocated per call)."""
    lib = _lib.load()
    assert emb.is_cuda and emb.dtype == torch.float32 and emb.is_contiguous() and rows.is_contiguous() and rows.dtype == torch.int64
    assert loss_acc.dtype == torch.float64 and (grad is None or (grad.dtype == torch.float32 and grad.is_contiguous() and grad.shape == emb.shape))
    n, d = emb.shape
    r, length = rows.shape
    if is_deterministic():
        if r == 0:
            return
        work = work or DetWork()
        ids, contrib, row_loss = position_grads(emb, rows, context_size, negative, scale, work)
        accumulate_det(ids, contrib, grad, touched, row_loss, scale, loss_acc, work.scratch)
        return
    with _lib.on_device(emb.device):
        check(lib.pope_n2v_loss_grad(ptr(emb), n, d, ptr(rows), r, length, context_size, 1 if negative else 0, scale, ptr(loss_acc),
                                     ptr(grad), ptr(touched), engine._stream()))


def sparse_adam(emb, grad, touched, exp_avg, exp_avg_sq, lr: float, beta1: float, beta2: float, eps: float, step: int) -> None:
    """torch.optim.SparseAdam on the rows flagged in ``touched``; their grad rows and flags are cleared (pope_n2v_sparse_adam)."""
    lib = _lib.load()
    n, d = emb.shape
    for t in (emb, grad, exp_avg, exp_avg_sq):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (n, d)
    assert touched.dtype == torch.uint8 and touched.numel() == n
    with _lib.on_device(emb.device):
        check(lib.pope_n2v_sparse_adam(ptr(emb), ptr(grad), ptr(touched), ptr(exp_avg), ptr(exp_avg_sq), n, d, lr, beta1, beta2, eps, step,
                                       engine._stream()))


def _terms(rows: torch.Tensor, context_size: int) -> int:
    return rows.shape[0] * (rows.shape[1] + 1 - context_size) * (context_size - 1)


class _SkipGramLoss(torch.autograd.Function):
    """pos.mean() + neg.mean() of PyG's loss; backward hands autograd the DENSE [N, D] gradient the same kernel accumulated."""

    @staticmethod
    def forward(ctx, weight, pos_rw, neg_rw):
        w = weight.detach().contiguous()
        acc = torch.zeros(1, dtype=torch.float64, device=w.device)
        need = weight.requires_grad
        grad = torch.zeros_like(w) if need else None
        touched = torch.zeros(w.shape[0], dtype=torch.uint8, device=w.device) if need else None
        work = DetWork()
        for rows, negative in ((pos_rw, False), (neg_rw, True)):
            if rows.shape[0]:
                loss_grad(w, rows, rows.shape[1], negative, 1.0 / _terms(rows, rows.shape[1]), acc, grad, touched, work)
        ctx.grad = grad
        return acc[0].to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        return ctx.grad * grad_out, None, None


class Node2Vec(torch.nn.Module):
    """``torch_geometric.nn.Node2Vec`` for first-order walks (``p == q == 1``), living on the GPU from construction.

    ``embedding.weight`` is ``torch.nn.Embedding(N, D)``'s table, initialised on the CPU (so it is a pure function of the torch CPU
    seed, as in PyG) and then moved.  ``sparse`` is accepted for the signature: :meth:`step` is always the sparse update, and
    :meth:`loss` always returns a dense gradient.  ``grad``, ``touched``, ``exp_avg``, ``exp_avg_sq`` and ``step_count`` -- the state of
    :meth:`step` -- live on the module, and so do the buffers of the deterministic mode (``_det``: sized on first use, regrown only
    for a larger batch, shared by the positive and the negative call of a step, which run on one stream in order).
    """

    def __init__(self, edge_index, embedding_dim, walk_length, context_size, walks_per_node=1, p=1, q=1, num_negative_samples=1,
                 num_nodes=None, sparse=False):
        super().__init__()
        assert walk_length >= context_size
        self._check_walk_parameters(p, q)
        dev =engine.require_gpu(edge_index.device if edge_index.is_cuda else None)
        n = int(edge_index.max()) + 1 if num_nodes is None else int(num_nodes)
        self.num_nodes, self.embedding_dim = n, int(embedding_dim)
        self.walk_length, self.context_size = int(walk_length), int(context_size)           # walk_length STEPS: a row has walk_length + 1 nodes (PyG takes one step fewer)
        self.walks_per_node, self.num_negative_samples = int(walks_per_node), int(num_negative_samples)
        self.p, self.q, self.sparse = p, q, sparse
        self.embedding = torch.nn.Embedding(n, self.embedding_dim, sparse=sparse)           # N(0, 1) from the CPU generator
        self.embedding.to(dev)
        self.csr = self._build_csr(edge_index.to(dev, torch.int64).contiguous(), n)
        with torch.cuda.device(dev):
            self.grad = torch.zeros(n, self.embedding_dim, device=dev)
            self.touched = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.exp_avg = torch.zeros_like(self.grad)
            self.exp_avg_sq = torch.zeros_like(self.grad)
            self._loss_acc = torch.zeros(1, dtype=torch.float64, device=dev)
        self._det = DetWork()
        self.step_count = 0
        self.lr, self.betas, self.eps = 0.01, (0.9, 0.999), 1e-8                            # torch.optim.SparseAdam's defaults, lr as the PyG examples

    @staticmethod
    def _check_walk_parameters(p, q) -> None:
        """Before anything needs a GPU.  This class draws first-order walks only and keeps saying so:
        :class:`SecondOrderNode2Vec` is the class that takes any finite ``p, q > 0``."""
        if p != 1 or q != 1:
            raise NotImplementedError(f"Node2Vec: only first-order walks (p = 1, q = 1) are implemented, got p = {p}, q = {q}: "
                                      "second-order (p/q-biased) walks are out of scope")

    @staticmethod
    def _build_csr(edge_index, num_nodes):
        return engine.build_csr(edge_index, num_nodes)

    @property
    def device(self):
        return self.embedding.weight.device

    def reset_parameters(self):
        with torch.no_grad():
            self.embedding.weight.copy_(torch.nn.Embedding(self.num_nodes, self.embedding_dim).weight)

    def forward(self, batch=None):
        emb = self.embedding.weight
        return emb if batch is None else emb.index_select(0, batch.to(emb.device))

    # ---- sampling ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _fresh_seed() -> int:
        return int(torch.randint(0, 1 << 62, (1,)))               # from torch's CPU generator, as PyG's samplers draw from torch's

    def walks(self, batch, seed: int, first_row: int = 0):
        """(pos rows [B * walks_per_node, L + 1], neg rows [B * walks_per_node * num_negative_samples, L + 1]) for ``seed``:
        the batch repeated as PyG repeats it (``batch.repeat(k)``)."""
        batch = _as_rows(torch.as_tensor(batch), self.device)
        starts = batch.repeat(self.walks_per_node)
        c = self.csr
        if self.num_negative_samples == 1:
            return walks(c.rowptr, c.col, self.num_nodes, starts, self.walk_length, seed, first_row)
        pos, _ = walks(c.rowptr, c.col, self.num_nodes, starts, self.walk_length, seed, first_row, negative=False)
        _, neg = walks(c.rowptr, c.col, self.num_nodes, batch.repeat(self.walks_per_node * self.num_negative_samples), self.walk_length, seed,
                       first_row, positive=False)
        return pos, neg

    def pos_sample(self, batch, seed=None):
        return windows(self.walks(batch, self._fresh_seed() if seed is None else seed)[0], self.context_size)

    def neg_sample(self, batch, seed=None):
        return windows(self.walks(batch, self._fresh_seed() if seed is None else seed)[1], self.context_size)

    def sample(self, batch, seed=None):
        pos, neg = self.walks(batch, self._fresh_seed() if seed is None else seed)
        return windows(pos, self.context_size), windows(neg, self.context_size)

    def _batches(self, batch_size, shuffle, generator):
        order = torch.randperm(self.num_nodes, generator=generator) if shuffle else torch.arange(self.num_nodes)
        order = order.to(self.device)
        return [order[lo:lo + batch_size] for lo in range(0, self.num_nodes, batch_size)]

    def loader(self, batch_size=1, shuffle=True, generator=None):
        """Yields ``(pos_rw, neg_rw)`` window matrices for batches of ``range(num_nodes)`` (PyG: a DataLoader with ``sample`` as collate_fn)."""
        for batch in self._batches(batch_size, shuffle, generator):
            yield self.sample(batch)

    # ---- loss ----------------------------------------------------------------------------------------------------------------
    def loss(self, pos_rw, neg_rw):
        """PyG's ``loss`` on window matrices ``[M, C]``: a float32 scalar with autograd support.  Its backward hands
        ``embedding.weight`` a DENSE ``[N, D]`` gradient out of the same kernel: this is the form for checking and for small graphs;
        training goes through :meth:`step`, which never materialises the windows or a dense gradient tensor per step."""
        dev = self.device
        pos_rw, neg_rw = _as_rows(pos_rw, dev), _as_rows(neg_rw, dev)
        for rw in (pos_rw, neg_rw):
            if rw.numel() and (int(rw.min()) < 0 or int(rw.max()) >= self.num_nodes):
                raise IndexError("Node2Vec.loss: node id outside [0, num_nodes)")
        return _SkipGramLoss.apply(self.embedding.weight, pos_rw, neg_rw)

    # ---- training ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, batch, seed: int):
        """One training step on ``batch`` without autograd: the walks and negatives of ``seed``, the loss and its gradient straight from
        the walk rows, SparseAdam on the touched rows.  Returns the loss (``pos.mean() + neg.mean()``) as a device scalar; nothing is
        read back."""
        pos, neg = self.walks(batch, seed)
        w = self.embedding.weight.data
        acc = self._loss_acc.zero_()
        c = self.context_size
        loss_grad(w, pos, c, False, 1.0 / _terms(pos, c), acc, self.grad, self.touched, self._det)
        loss_grad(w, neg, c, True, 1.0 / _terms(neg, c), acc, self.grad, self.touched, self._det)
        self.step_count += 1
        sparse_adam(w, self.grad, self.touched, self.exp_avg, self.exp_avg_sq, self.lr, self.betas[0], self.betas[1], self.eps,
                    self.step_count)
        return acc[0].to(torch.float32)

    def fit(self, epochs, batch_size=128, lr=0.01, seed=0, shuffle=True, on_epoch=None):
        """``epochs`` passes of :meth:`step` over every node; returns the per-epoch mean of the step losses (one read-back per epoch).
        ``on_epoch(epoch, loss)``, if given, is called after every epoch; it must leave the model and torch's generators alone."""
        self.lr = float(lr)
        gen = torch.Generator().manual_seed(int(seed))
        losses = []
        for _ in range(int(epochs)):
            total = torch.zeros((), device=self.device)
            batches = self._batches(batch_size, shuffle, gen)
            for batch in batches:
                total += self.step(batch, ((int(seed) << 32) + self.step_count) & _MASK64)
            losses.append(float(total) / max(len(batches), 1))
            if on_epoch is not None:
                on_epoch(len(losses) - 1, losses[-1])
        return losses

    # ---- evaluation ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def test(self, train_z, train_y, test_z, test_y, solver='lbfgs', multi_class='auto', *args, **kwargs):
        """PyG's ``test``: the accuracy on ``(test_z, test_y)`` of a logistic regression fitted on ``(train_z, train_y)``, as
        ``LogisticRegression(solver=solver, *args, **kwargs).fit(train_z, train_y).score(test_z, test_y)`` computes it, with the
        objective and the predictions on the GPU (logreg.py).  ``z``: float32, CPU or device.  Accepted: ``solver='lbfgs'``,
        ``multi_class='auto'`` and the keywords ``C``, ``fit_intercept``, ``max_iter``, ``tol``; anything else raises
        ``NotImplementedError`` before a GPU is needed."""
        from . import logreg
        kw = logreg.check_test_arguments(solver, multi_class, args, kwargs)
        return logreg.score(logreg.fit(train_z, train_y, **kw), test_z, test_y)

    @torch.no_grad()
    def test_nodes(self, train_idx, test_idx, y, **kwargs):
        """:meth:`test` on ``embedding.weight`` through row ids: ``test(z[train_idx], y[train_idx], z[test_idx], y[test_idx])``
        without the ``z[mask]`` copies.  ``y``: one label per node."""
        from . import logreg
        kw = logreg.check_test_arguments(kwargs=kwargs)
        z = self.embedding.weight.detach()
        y = torch.as_tensor(y).reshape(-1).cpu()
        train_idx, test_idx = (torch.as_tensor(i).reshape(-1).to('cpu', torch.int64) for i in (train_idx, test_idx))
        model = logreg.fit(z, y[train_idx], ids=train_idx, **kw)
        return logreg.score(model, z, y[test_idx], ids=test_idx)


class SecondOrderNode2Vec(Node2Vec):
    """:class:`Node2Vec` with node2vec's second-order walks: any finite ``p, q > 0`` (``ValueError`` otherwise, before a GPU is
    needed).  After a step ``t -> v`` a neighbour ``x`` of ``v`` weighs ``1 / p`` if ``x == t``, ``1`` if ``t -> x`` is an edge and
    ``1 / q`` otherwise (pope_n2v_walks_biased; torch_cluster tests ``x -> t``: the same on a symmetric graph).  The CSR is the
    canonical one (``engine.build_csr_canonical``: every row ascending), which the kernel's edge test needs; ``p = q = 1`` is legal
    and gives the first-order walks on that CSR.  Negative rows, windows, loss, :meth:`step`, :meth:`fit` and the deterministic
    mode are inherited unchanged.

    A subclass only because ``Node2Vec(..., p != 1 or q != 1)`` is pinned to raise ``NotImplementedError`` without a GPU."""

    @staticmethod
    def _check_walk_parameters(p, q) -> None:
        _check_pq(p, q)

    @staticmethod
    def _build_csr(edge_index, num_nodes):
        return engine.build_csr_canonical(edge_index, num_nodes)

    def walks(self, batch, seed: int, first_row: int = 0):
        """As :meth:`Node2Vec.walks`: biased positive rows, and the negative rows of the first-order launch."""
        batch = _as_rows(torch.as_tensor(batch), self.device)
        c = self.csr
        pos = walks_biased(c.rowptr, c.col, self.num_nodes, batch.repeat(self.walks_per_node), self.walk_length, seed, self.p, self.q,
                           first_row)
        _, neg = walks(c.rowptr, c.col, self.num_nodes, batch.repeat(self.walks_per_node * self.num_negative_samples), self.walk_length,
                       seed, first_row, positive=False)
        return pos, neg
