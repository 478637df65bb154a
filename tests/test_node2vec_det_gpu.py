"""node2vec in the library's deterministic mode, on the device: pope_n2v_accumulate_det bit for bit against the NumPy restatement of
its contract on lists whose sum shows its order, the fixed-order loss sum, pope_n2v_position_grads against torch float64 and against
itself (two calls, a sub-batch), loss_grad / Node2Vec.loss through the mode, and what the mode is for: Node2Vec.fit and the
generator's command line give the same bits twice under one seed.

Shapes, graphs, torch references and the parity yardstick (error at most 2 x torch float32's + 1e-6) are those of
tests/test_node2vec_gpu.py.  Every test starts and ends with the mode off (the `mode_off` fixture)."""
import numpy as np
import pytest
import torch

import node2vec_det_cases as cases
from test_node2vec_gpu import (C4, GRAD_FACTOR, L7, N70, _assert_no_worse_than_torch, _check_loss_and_grad, _community_graph, _graph70,
                               _starts201, _torch_loss_and_grad, _walk_form, _walks, _windows)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


@pytest.fixture(scope="module")
def g70(dev):
    from graphpope_amd import engine
    ei = _graph70()
    return ei, engine.build_csr(torch.as_tensor(ei, device=dev), N70)


@pytest.fixture(autouse=True)
def mode_off():
    from graphpope_amd import sage
    assert not sage.is_deterministic(), "an earlier test left the switch on"
    yield
    sage.set_deterministic(False)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _terms(rows, c):
    return rows.shape[0] * (rows.shape[1] + 1 - c) * (c - 1)


# ---- 1. the ordered sum ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 96, 128, 256])
def test_ordered_sum_is_exact(dev, d):
    from graphpope_amd import node2vec
    ids, contrib, prior = cases.ordered_sum_case(d)
    ids_t, contrib_t = torch.from_numpy(ids).to(dev), torch.from_numpy(contrib).to(dev)
    grad = torch.from_numpy(prior).to(dev)
    touched = torch.zeros(cases.N, dtype=torch.uint8, device=dev)
    scratch = torch.empty(_scratch_bytes(cases.M, cases.N), dtype=torch.uint8, device=dev)
    now = prior
    for m in (cases.M, 200, 1):                                     # the same buffers again: nothing of the earlier index is read
        want, want_touched = cases.accumulate_reference(ids[:m], contrib[:m], now)
        touched.zero_()
        node2vec.accumulate_det(ids_t[:m], contrib_t[:m], grad, touched, None, 1.0, None, scratch)
        got = grad.cpu().numpy()
        assert np.array_equal(touched.cpu().numpy(), want_touched), m   # exactly the nodes with a valid entry
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (m, int((got.view(np.int32) != want.view(np.int32)).sum()))
        idle = want_touched == 0
        assert idle.any() and np.array_equal(got[idle].view(np.int32), now[idle].view(np.int32))   # other rows: bit-unchanged
        now = want
    assert want_touched.sum() == (1 if 0 <= ids[0] < cases.N else 0)


def test_ordered_sum_carries_the_index_scan_over_its_rounds(dev):
    """N = 2 x 8192 + 3, so the one-block scan of the index takes three rounds: entries only at nodes 0, 8191 | 8192, 16383 | 16384 and
    16386 (and a few outside [0, N)).  Where a list behind a round edge begins is the carry of the rounds before."""
    from graphpope_amd import node2vec
    ids, contrib, prior = cases.scan_carry_case(32)
    want, want_touched = cases.accumulate_reference(ids, contrib, prior)
    grad = torch.from_numpy(prior).to(dev)
    touched = torch.zeros(cases.CARRY_N, dtype=torch.uint8, device=dev)
    scratch = torch.empty(_scratch_bytes(cases.CARRY_M, cases.CARRY_N), dtype=torch.uint8, device=dev)
    node2vec.accumulate_det(torch.from_numpy(ids).to(dev), torch.from_numpy(contrib).to(dev), grad, touched, None, 1.0, None, scratch)
    got = grad.cpu().numpy()
    assert sorted(np.nonzero(want_touched)[0]) == sorted(cases.CARRY_LISTS)
    assert np.array_equal(touched.cpu().numpy(), want_touched)      # exactly the six nodes
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), int((got.view(np.int32) != want.view(np.int32)).sum())


def _scratch_bytes(m, n):
    from graphpope_amd import _lib
    return _lib.load().pope_n2v_accumulate_det_scratch_bytes(m, n)


# ---- 2. the loss sum ---------------------------------------------------------------------------------------------------------
def test_loss_sum_is_reproducible_and_accurate(dev):
    from graphpope_amd import node2vec
    rng = np.random.default_rng(3)
    r, scale = 2500, 1.0 / 7.0                                       # more than one round of the block, no multiple of its size
    row_loss = (rng.random(r) * 10.0 ** rng.uniform(-3, 3, r))
    row_loss_t = torch.from_numpy(row_loss).to(dev)
    none_i, none_c = torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, 32, device=dev)
    results = []
    for _ in range(3):
        acc = torch.zeros(1, dtype=torch.float64, device=dev)
        for _ in range(2):
            node2vec.accumulate_det(none_i, none_c, None, None, row_loss_t, scale, acc)
        results.append(acc.clone())
    assert all(torch.equal(results[0].view(torch.int64), x.view(torch.int64)) for x in results[1:])
    ref64 = torch.tensor([2.0 * scale * float(np.sum(row_loss))], dtype=torch.float64, device=dev)
    ref32 = 2.0 * scale * row_loss_t.float().sum().reshape(1)
    _assert_no_worse_than_torch(results[0], ref32, ref64, "loss sum")
    # row_loss = NULL: the gradient part alone, loss_acc untouched
    ids, contrib, prior = cases.ordered_sum_case(32)
    acc = torch.full((1,), 3.25, dtype=torch.float64, device=dev)
    grad, touched = torch.from_numpy(prior).to(dev), torch.zeros(cases.N, dtype=torch.uint8, device=dev)
    node2vec.accumulate_det(torch.from_numpy(ids).to(dev), torch.from_numpy(contrib).to(dev), grad, touched, None, scale, acc)
    assert float(acc) == 3.25 and touched.any()


# ---- 3. the contributions ----------------------------------------------------------------------------------------------------
def _model(dev, ei, dim, seed):
    from graphpope_amd.node2vec import Node2Vec
    torch.manual_seed(seed)
    return Node2Vec(torch.as_tensor(ei, device=dev), dim, walk_length=L7, context_size=C4, num_nodes=N70)


def _segment_sum(ids, contrib, n):
    out = torch.zeros(n, contrib.shape[1], dtype=torch.float64, device=contrib.device)
    keep = ids >= 0
    return out.index_add_(0, ids[keep].long(), contrib[keep].double())


def _check_contributions(dev, w, pos, neg, what):
    """ids, and loss and gradient rebuilt on the host in float64 from row_loss and contrib, against torch on the window matrices."""
    from graphpope_amd import node2vec
    loss64, grad64 = _torch_loss_and_grad(w, _windows(pos, C4), _windows(neg, C4), torch.float64)
    loss32, grad32 = _torch_loss_and_grad(w, _windows(pos, C4), _windows(neg, C4), torch.float32)
    loss = torch.zeros((), dtype=torch.float64, device=dev)
    grad = torch.zeros(N70, w.shape[1], dtype=torch.float64, device=dev)
    outs = []
    for rows, negative in ((pos, False), (neg, True)):
        scale = 1.0 / _terms(rows, C4)
        ids, contrib, row_loss = node2vec.position_grads(w, rows, C4, negative, scale)
        assert ids.dtype == torch.int32 and contrib.shape == (rows.numel(), w.shape[1]) and row_loss.shape == (rows.shape[0],)
        assert torch.equal(ids.long(), rows.flatten())
        loss += scale * row_loss.sum()
        grad += _segment_sum(ids, contrib, N70)
        again = node2vec.position_grads(w, rows, C4, negative, scale)
        assert torch.equal(_bits(again[1]), _bits(contrib)) and torch.equal(again[2].view(torch.int64), row_loss.view(torch.int64))
        part = node2vec.position_grads(w, rows[50:100].contiguous(), C4, negative, scale)     # no dependence on R
        assert torch.equal(_bits(part[1]), _bits(contrib[50 * (L7 + 1):100 * (L7 + 1)]))
        assert torch.equal(part[2].view(torch.int64), row_loss[50:100].view(torch.int64))
        outs.append((ids, contrib, row_loss))
    _assert_no_worse_than_torch(loss, loss32, loss64, f"{what} loss from row_loss")
    _assert_no_worse_than_torch(grad, grad32, grad64, f"{what} gradient from contrib", GRAD_FACTOR)
    return outs


@pytest.mark.parametrize("dim", [32, 128])
def test_contributions_match_torch(dev, g70, dim):
    from graphpope_amd import node2vec
    ei, csr = g70
    m = _model(dev, ei, dim, dim)
    with torch.no_grad():
        m.embedding.weight.mul_(2.0 / dim ** 0.5)
    w = m.embedding.weight.detach()
    pos, neg = _walks(csr, N70, _starts201(dev), L7, seed=21)
    _check_contributions(dev, w, pos, neg, f"D = {dim}")
    # a row with an id outside [0, N): all its ids -1, its loss 0; the other rows as before
    bad = pos.clone()
    bad[3, 5], bad[77, 0] = N70, -1
    ids, contrib, row_loss = node2vec.position_grads(w, bad, C4, False, 1.0)
    good_ids, good_contrib, good_loss = node2vec.position_grads(w, pos, C4, False, 1.0)
    ids, good_ids = ids.view(-1, L7 + 1), good_ids.view(-1, L7 + 1)
    assert (ids[[3, 77]] == -1).all() and (row_loss[[3, 77]] == 0).all() and (good_loss[[3, 77]] > 0).all()
    rest = torch.ones(pos.shape[0], dtype=torch.bool, device=dev)
    rest[[3, 77]] = False
    assert torch.equal(ids[rest], good_ids[rest]) and torch.equal(row_loss[rest].view(torch.int64), good_loss[rest].view(torch.int64))
    assert torch.equal(_bits(contrib.view(pos.shape[0], -1)[rest]), _bits(good_contrib.view(pos.shape[0], -1)[rest]))


def test_contributions_with_saturated_products(dev, g70):
    ei, csr = g70
    m = _model(dev, ei, 128, 7)
    w = m.embedding.weight
    with torch.no_grad():
        off_diagonal = 1.0 - torch.eye(N70, dtype=torch.float64, device=dev)
        w.mul_(float((40.0 / (w.double() @ w.double().T * off_diagonal).abs().max()) ** 0.5))
        products = w.double() @ w.double().T * off_diagonal
    assert 39.0 < float(products.abs().max()) < 41.0 and float(products.min()) < -25.0
    pos, neg = _walks(csr, N70, _starts201(dev), L7, seed=22)
    _check_contributions(dev, w.detach(), pos, neg, "saturated")


# ---- 4. through the mode -----------------------------------------------------------------------------------------------------
def _check_through_the_mode(model, pos, neg, what):
    from graphpope_amd import sage
    w = model.embedding.weight
    pos_rw, neg_rw = _windows(pos, C4), _windows(neg, C4)
    with sage.deterministic():
        _check_loss_and_grad(model, pos, neg, C4, what + ", deterministic")     # yardstick against torch, touched == the rows that occur
        walk = [_walk_form(w.detach(), pos, neg, C4) for _ in range(2)]
        window = []
        for _ in range(2):
            w.grad = None
            loss = model.loss(pos_rw, neg_rw)
            loss.backward()
            window.append((loss.detach().clone(), w.grad.clone()))
        w.grad = None
    assert torch.equal(_bits(walk[0][1]), _bits(walk[1][1])) and torch.equal(walk[0][0].view(torch.int64), walk[1][0].view(torch.int64))
    assert torch.equal(walk[0][2], walk[1][2])
    assert torch.equal(_bits(window[0][1]), _bits(window[1][1])) and torch.equal(_bits(window[0][0]), _bits(window[1][0]))
    assert not sage.is_deterministic()


@pytest.mark.parametrize("dim", [32, 128])
def test_loss_grad_through_the_mode_on_g70(dev, g70, dim):
    ei, csr = g70
    m = _model(dev, ei, dim, dim)
    with torch.no_grad():
        m.embedding.weight.mul_(2.0 / dim ** 0.5)
    starts = _starts201(dev)
    pos, neg = _walks(csr, N70, starts, L7, seed=21)
    pos, neg = pos[starts != 69], neg[starts != 69]                              # node 69 occurs in neither: a row that stays untouched
    neg = torch.where(neg == 69, torch.zeros_like(neg), neg)
    _check_through_the_mode(m, pos, neg, f"D = {dim}")


def test_loss_grad_through_the_mode_on_the_two_cycle(dev):
    """100 rows of 8 positions over two nodes: 800 entries on each, per call."""
    from graphpope_amd.node2vec import Node2Vec
    torch.manual_seed(2)
    m = Node2Vec(torch.tensor([[0, 1], [1, 0]], device=dev), 32, walk_length=L7, context_size=C4, walks_per_node=50, num_nodes=2)
    with torch.no_grad():
        m.embedding.weight.mul_(0.4)
    pos, neg = m.walks(torch.tensor([0, 1], device=dev), seed=4)
    assert pos.shape == (100, L7 + 1)
    _check_through_the_mode(m, pos, neg, "two-cycle")


# ---- 5. training is a function of the seed -----------------------------------------------------------------------------------
def _fit(dev, seed):
    from graphpope_amd.node2vec import Node2Vec
    torch.manual_seed(0)
    m = Node2Vec(torch.as_tensor(_community_graph(0), device=dev), 32, walk_length=10, context_size=5, walks_per_node=4,
                 num_negative_samples=1, num_nodes=512)
    return m, m.fit(epochs=2, batch_size=64, lr=0.05, seed=seed)


def test_training_is_a_function_of_the_seed(dev):
    from graphpope_amd import sage
    with sage.deterministic():
        (a, loss_a), (b, loss_b), (c, loss_c) = _fit(dev, 0), _fit(dev, 0), _fit(dev, 1)
    assert loss_a == loss_b and len(loss_a) == 2 and all(np.isfinite(loss_a))
    for name in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert torch.equal(_bits(a.embedding.weight.detach()), _bits(b.embedding.weight.detach()))
    for m in (a, b, c):
        assert not m.grad.any() and not m.touched.any() and m.step_count == 16
    assert loss_c != loss_a and not torch.equal(c.embedding.weight.detach(), a.embedding.weight.detach())


# ---- 6. the command line -----------------------------------------------------------------------------------------------------
def test_generator_writes_the_same_table_twice(dev, tmp_path, monkeypatch):
    from graphpope_amd import generate_node2vec_embedding as gen, sage
    n = 512
    ei = _community_graph(0)
    x = np.random.default_rng(1).random((n, 12), dtype=np.float32)
    mask = np.ones(n, dtype=bool)
    np.savez(tmp_path / "pubmed.npz", x=x, y=np.arange(n) % 3, edge_index=ei, train_mask=mask, val_mask=mask, test_mask=mask)
    monkeypatch.setenv("GRAPHPOPE_DETERMINISTIC", "1")
    tables = []
    for k in range(2):
        out = tmp_path / f"table{k}.pt"
        gen.main(["--dataset", "pubmed", "--epochs", "1", "--data_dir", str(tmp_path), "--out", str(out)])
        assert not sage.is_deterministic()                                         # the mode is off afterwards
        tables.append(torch.load(out))
    assert tables[0].shape == (n, 128) and tables[0].dtype == torch.float32 and torch.isfinite(tables[0]).all()
    assert torch.equal(_bits(tables[0]), _bits(tables[1]))
    torch.manual_seed(42)
    assert not torch.equal(tables[0], torch.nn.Embedding(n, 128).weight.detach())   # it did train
