"""node2vec on the GPU (graphpope_amd.node2vec over pope_n2v_walks / _windows / _loss_grad / _sparse_adam): exact properties of the
walks, their reproducibility and uniformity, the window matrices, the loss and its gradient against PyG's ``loss`` restated in plain
torch, SparseAdam against torch.optim.SparseAdam, a training run that has to learn, and the generator's command line handing its
table to ``Graphpope(embedding_space='node2vec')``.

Parity with torch is judged as tests/test_clip_gpu.py judges it: the error against the same torch code on float64 copies, relative to
the largest float64 magnitude, may be at most twice the error of torch's float32 run, plus 1e-6.  No test compares the gradients of
two runs bit for bit: float atomic adds land in arrival order."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-15
N70, L7, C4 = 70, 7, 4


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


def _graph70():
    """70 nodes, directed.  0: hub of out-degree 100 (every target 10..59 twice).  1: out-degree 0 with in-edges.  3: self-loop.
    4 -> 5 twice (a repeated edge).  7 <-> 8: a 2-node cycle with no other way out.  69: isolated.  The rest: a ring with chords."""
    e = [(0, 10 + t % 50) for t in range(100)]
    e += [(2, 1), (2, 3), (3, 3), (3, 1), (3, 4), (4, 5), (4, 5), (4, 6), (5, 0), (6, 4), (6, 2), (7, 8), (8, 7), (9, 7), (9, 10)]
    for v in range(10, 69):
        e += [(v, 10 + (v - 9) % 59), (v, 10 + (v * 7) % 59)]
        if v % 5 == 0:
            e.append((v, (1, 7, 3, 4, 0, 9, 2)[(v // 5) % 7]))
    ei = np.array(e, dtype=np.int64).T
    return ei[:, np.random.default_rng(0).permutation(ei.shape[1])]              # not sorted by source


@pytest.fixture(scope="module")
def g70(dev):
    from graphpope_amd import engine
    ei = _graph70()
    csr = engine.build_csr(torch.as_tensor(ei, device=dev), N70)
    deg = np.bincount(ei[0], minlength=N70)
    assert deg[0] == 100 and deg[1] == 0 and deg[69] == 0 and not (ei[1] == 69).any() and (ei[1] == 1).any()
    return ei, csr, deg


def _starts201(dev):
    s = (torch.arange(201) * 37) % N70                                            # every node, with repeats; 201 is no multiple of 64
    s[:6] = torch.tensor([7, 8, 1, 69, 0, 3])
    return s.to(dev)


def _walks(csr, n, starts, length, seed, first_row=0, neg=True):
    from graphpope_amd import node2vec
    return node2vec.walks(csr.rowptr, csr.col, n, starts, length, seed, first_row, negative=neg)


# ---- walks -------------------------------------------------------------------------------------------------------------------
def test_walks_exact_properties(dev, g70):
    ei, csr, deg = g70
    starts = _starts201(dev)
    pos, neg = _walks(csr, N70, starts, L7, seed=11)
    assert pos.shape == (201, L7 + 1) and neg.shape == (201, L7 + 1) and pos.dtype == neg.dtype == torch.int64 and pos.is_cuda
    assert torch.equal(pos[:, 0], starts) and torch.equal(neg[:, 0], starts)
    p, s = pos.cpu().numpy(), starts.cpu().numpy()
    edges = set(zip(ei[0].tolist(), ei[1].tolist()))
    for row in p:
        for a, b in zip(row[:-1], row[1:]):
            assert (a, b) in edges or (a == b and deg[a] == 0), (a, b)
    for row in p[(s == 7) | (s == 8)]:
        assert all(row[k + 1] == 15 - row[k] for k in range(L7)), row            # 7, 8, 7, 8, ...
    assert (p[s == 1] == 1).all() and (p[s == 69] == 69).all()                    # nowhere to go: stay
    assert len(set(p[s == 0][:, 1].tolist())) > 1                                 # the hub's rows do not all take the same slot
    q = neg.cpu().numpy()
    assert q.min() >= 0 and q.max() < N70 and len(np.unique(q[:, 1:])) > N70 // 2


def test_walks_are_reproducible_and_rows_do_not_depend_on_the_call(dev, g70):
    _, csr, _ = g70
    starts = _starts201(dev)
    pos, neg = _walks(csr, N70, starts, L7, seed=11)
    pos2, neg2 = _walks(csr, N70, starts, L7, seed=11)
    assert torch.equal(pos, pos2) and torch.equal(neg, neg2)
    pos3, neg3 = _walks(csr, N70, starts, L7, seed=12)
    assert not torch.equal(pos, pos3) and not torch.equal(neg, neg3)
    part_pos, part_neg = _walks(csr, N70, starts[50:100], L7, seed=11, first_row=50)
    assert torch.equal(part_pos, pos[50:100]) and torch.equal(part_neg, neg[50:100])
    only_pos, none = _walks(csr, N70, starts, L7, seed=11, neg=False)
    assert none is None and torch.equal(only_pos, pos)


UNIFORM_SEEDS = [20260101, 1, 2, 3]        # a fixed seed, and three more to show that passing is no accident
UNIFORM_B = 65536


@pytest.mark.parametrize("seed", UNIFORM_SEEDS)
def test_one_step_from_a_hub_is_uniform(dev, seed):
    """65 536 one-step walks from a hub with 100 distinct targets: every count within 6 sigma of B / d, sigma = sqrt(B (1/d)(1 - 1/d))
    (a binomial count; 100 cells at 6 sigma: a false alarm about once in 5 million seeds)."""
    from graphpope_amd import engine
    d = 100
    ei = torch.stack([torch.zeros(d, dtype=torch.int64), torch.arange(1, d + 1)]).to(dev)
    csr = engine.build_csr(ei, d + 1)
    pos, _ = _walks(csr, d + 1, torch.zeros(UNIFORM_B, dtype=torch.int64, device=dev), 1, seed, neg=False)
    counts = torch.bincount(pos[:, 1], minlength=d + 1).cpu().numpy()
    assert counts[0] == 0 and counts.sum() == UNIFORM_B
    sigma = np.sqrt(UNIFORM_B * (1 / d) * (1 - 1 / d))
    dev_max = np.abs(counts[1:] - UNIFORM_B / d).max()
    print(f"seed {seed}: largest deviation {dev_max:.1f} = {dev_max / sigma:.2f} sigma")
    assert dev_max <= 6 * sigma


@pytest.mark.parametrize("seed", UNIFORM_SEEDS)
def test_two_steps_on_k8_are_independent(dev, seed):
    """65 536 two-step walks from node 0 of K_8: the 7 x 7 table of (first step, slot of the second step) within 6 sigma per cell of
    B / 49.  A draw keyed on the row but not on the step would put everything on the diagonal of the slot table."""
    from graphpope_amd import engine
    n = 8
    src, dst = np.nonzero(~np.eye(n, dtype=bool))
    csr = engine.build_csr_canonical(torch.as_tensor(np.stack([src, dst]), device=dev), n)
    pos, _ = _walks(csr, n, torch.zeros(UNIFORM_B, dtype=torch.int64, device=dev), 2, seed, neg=False)
    p = pos.cpu().numpy()
    first, second = p[:, 1], p[:, 2]
    assert (first != 0).all() and (second != first).all()
    slot = second - (second > first)                                              # rank of the second node among first's 7 neighbours
    table = np.zeros((n, 7), dtype=np.int64)
    np.add.at(table, (first, slot), 1)
    table = table[1:]
    prob = 1 / 49
    sigma = np.sqrt(UNIFORM_B * prob * (1 - prob))
    dev_max = np.abs(table - UNIFORM_B * prob).max()
    print(f"seed {seed}: largest deviation {dev_max:.1f} = {dev_max / sigma:.2f} sigma")
    assert table.sum() == UNIFORM_B and dev_max <= 6 * sigma


def test_pos_and_neg_sample_are_the_windows_of_the_walk_rows(dev, g70):
    from graphpope_amd.node2vec import Node2Vec
    ei, _, _ = g70
    m = Node2Vec(torch.as_tensor(ei, device=dev), 32, walk_length=L7, context_size=C4, walks_per_node=3, num_negative_samples=2,
                 num_nodes=N70)
    batch = torch.tensor([0, 7, 1, 69, 3, 4, 12, 13, 14, 20, 33, 33, 50, 68, 9, 2, 5], device=dev)
    pos, neg = m.walks(batch, seed=5)
    assert torch.equal(pos[:, 0], batch.repeat(3)) and torch.equal(neg[:, 0], batch.repeat(6))
    n_win = L7 + 2 - C4
    want_pos = torch.cat([pos[:, j:j + C4] for j in range(n_win)], 0)
    want_neg = torch.cat([neg[:, j:j + C4] for j in range(n_win)], 0)
    assert want_pos.shape == (17 * 3 * n_win, C4) and want_neg.shape == (17 * 3 * 2 * n_win, C4)
    got_pos, got_neg = m.pos_sample(batch, seed=5), m.neg_sample(batch, seed=5)
    assert torch.equal(got_pos, want_pos) and torch.equal(got_neg, want_neg)
    both = m.sample(batch, seed=5)
    assert torch.equal(both[0], want_pos) and torch.equal(both[1], want_neg)
    torch.manual_seed(3)
    a = m.pos_sample(batch)
    torch.manual_seed(3)
    assert torch.equal(a, m.pos_sample(batch)) and a.shape == want_pos.shape     # without a seed: drawn from torch's CPU generator
    pairs = list(m.loader(batch_size=32, shuffle=False))
    assert len(pairs) == 3 and pairs[0][0].shape == (32 * 3 * n_win, C4) and pairs[2][1].shape == (6 * 3 * 2 * n_win, C4)


# ---- loss and gradient -------------------------------------------------------------------------------------------------------
def _pyg_loss(weight, pos_rw, neg_rw):
    """torch_geometric.nn.Node2Vec.loss, with F.embedding in place of the module's table."""
    d = weight.shape[1]
    terms = []
    for rw, negative in ((pos_rw, False), (neg_rw, True)):
        start, rest = rw[:, 0], rw[:, 1:].contiguous()
        h_start = F.embedding(start, weight).view(rw.size(0), 1, d)
        h_rest = F.embedding(rest.view(-1), weight).view(rw.size(0), -1, d)
        out = (h_start * h_rest).sum(dim=-1).view(-1)
        terms.append(-torch.log((1 - torch.sigmoid(out) if negative else torch.sigmoid(out)) + EPS).mean())
    return terms[0] + terms[1]


def _torch_loss_and_grad(weight, pos_rw, neg_rw, dtype):
    w = weight.detach().to(dtype).requires_grad_(True)
    loss = _pyg_loss(w, pos_rw, neg_rw)
    loss.backward()
    return loss.detach(), w.grad.detach()


def _rel_err(a, ref64):
    return float((a.double() - ref64).abs().max()) / max(float(ref64.abs().max()), 1e-300)


GRAD_FACTOR = 2.0


def _assert_no_worse_than_torch(mine, ref32, ref64, what, factor=2.0):
    e_mine, e_torch = _rel_err(mine, ref64), _rel_err(ref32, ref64)
    print(f"{what}: this {e_mine:.3e} torch float32 {e_torch:.3e}")
    assert e_mine <= factor * e_torch + 1e-6, (what, e_mine, e_torch)


def _windows(rows, c):
    return torch.cat([rows[:, j:j + c] for j in range(rows.shape[1] + 1 - c)], 0).contiguous()


def _walk_form(weight, pos, neg, c):
    """The fast form: loss and gradient straight from the walk rows (two pope_n2v_loss_grad calls), no autograd."""
    from graphpope_amd import node2vec
    acc = torch.zeros(1, dtype=torch.float64, device=weight.device)
    grad = torch.zeros_like(weight)
    touched = torch.zeros(weight.shape[0], dtype=torch.uint8, device=weight.device)
    for rows, negative in ((pos, False), (neg, True)):
        node2vec.loss_grad(weight, rows, c, negative, 1.0 / (rows.shape[0] * (rows.shape[1] + 1 - c) * (c - 1)), acc, grad, touched)
    return acc[0], grad, touched


def _check_loss_and_grad(model, pos, neg, c, what):
    """Window form through Node2Vec.loss(...).backward() and walk form through the kernel, both against torch on the window matrices."""
    w = model.embedding.weight
    pos_rw, neg_rw = _windows(pos, c), _windows(neg, c)
    loss64, grad64 = _torch_loss_and_grad(w, pos_rw, neg_rw, torch.float64)
    loss32, grad32 = _torch_loss_and_grad(w, pos_rw, neg_rw, torch.float32)
    assert torch.isfinite(loss64) and torch.isfinite(grad64).all()
    w.grad = None
    loss = model.loss(pos_rw, neg_rw)                                            # C == len: one window per row
    assert loss.dtype == torch.float32 and loss.dim() == 0 and torch.isfinite(loss)
    loss.backward()
    assert w.grad is not None and w.grad.shape == w.shape and torch.isfinite(w.grad).all()
    _assert_no_worse_than_torch(loss.detach(), loss32, loss64, f"{what} loss, window form")
    _assert_no_worse_than_torch(w.grad, grad32, grad64, f"{what} gradient, window form", GRAD_FACTOR)
    loss_w, grad_w, touched = _walk_form(w.detach(), pos, neg, c)                # C < len: the windows are never materialised
    _assert_no_worse_than_torch(loss_w, loss32, loss64, f"{what} loss, walk form")
    _assert_no_worse_than_torch(grad_w, grad32, grad64, f"{what} gradient, walk form", GRAD_FACTOR)
    seen = torch.zeros(w.shape[0], dtype=torch.bool, device=w.device)
    seen[torch.cat([pos.flatten(), neg.flatten()])] = True
    assert torch.equal(touched.bool(), seen)                                     # flagged exactly the rows that occur
    assert not grad_w[~seen].any() and not w.grad[~seen].any()
    w.grad = None
    (3.0 * model.loss(pos_rw, neg_rw)).backward()                                # the upstream gradient is applied
    assert float((w.grad - 3.0 * grad_w).abs().max()) <= 1e-5 * float((3.0 * grad_w).abs().max())
    w.grad = None
    return float(loss64)


@pytest.mark.parametrize("dim", [32, 128])
def test_loss_and_gradient_match_torch(dev, g70, dim):
    from graphpope_amd.node2vec import Node2Vec
    ei, csr, _ = g70
    torch.manual_seed(dim)
    m = Node2Vec(torch.as_tensor(ei, device=dev), dim, walk_length=L7, context_size=C4, num_nodes=N70)
    with torch.no_grad():
        m.embedding.weight.mul_(2.0 / dim ** 0.5)                                # products of order 1: neither branch saturates
    starts = _starts201(dev)
    pos, neg = _walks(csr, N70, starts, L7, seed=21)
    pos, neg = pos[starts != 69], neg[starts != 69]                              # node 69 occurs in neither: a row that stays untouched
    assert not (pos == 69).any() and pos.shape[0] > 190
    neg = torch.where(neg == 69, torch.zeros_like(neg), neg)
    _check_loss_and_grad(m, pos, neg, C4, f"D = {dim}")


def test_loss_on_the_two_cycle_where_start_and_context_collide(dev):
    from graphpope_amd.node2vec import Node2Vec
    torch.manual_seed(2)
    m = Node2Vec(torch.tensor([[0, 1], [1, 0]], device=dev), 32, walk_length=L7, context_size=C4, walks_per_node=50, num_nodes=2)
    with torch.no_grad():
        m.embedding.weight.mul_(0.4)
    pos, neg = m.walks(torch.tensor([0, 1], device=dev), seed=4)
    assert pos.shape == (100, L7 + 1) and (neg[:, 1:] == neg[:, :1]).any()       # windows whose start is its own context
    _check_loss_and_grad(m, pos, neg, C4, "two-cycle")


def test_loss_with_saturated_products(dev, g70):
    """Products up to +-40: sigmoid(out) + 1e-15 and 1 - sigmoid(out) + 1e-15 both reach the point where only the 1e-15 is left."""
    from graphpope_amd.node2vec import Node2Vec
    ei, csr, _ = g70
    torch.manual_seed(7)
    m = Node2Vec(torch.as_tensor(ei, device=dev), 128, walk_length=L7, context_size=C4, num_nodes=N70)
    w = m.embedding.weight
    with torch.no_grad():
        off_diagonal = 1.0 - torch.eye(N70, dtype=torch.float64, device=dev)       # products of two different nodes
        w.mul_(float((40.0 / (w.double() @ w.double().T * off_diagonal).abs().max()) ** 0.5))
        products = w.double() @ w.double().T * off_diagonal
    assert 39.0 < float(products.abs().max()) < 41.0 and float(products.min()) < -25.0
    pos, neg = _walks(csr, N70, _starts201(dev), L7, seed=22)
    loss64 = _check_loss_and_grad(m, pos, neg, C4, "saturated")
    assert np.isfinite(loss64) and loss64 > 1.0


def test_loss_refuses_ids_outside_the_table(dev):
    from graphpope_amd.node2vec import Node2Vec
    m = Node2Vec(torch.tensor([[0, 1], [1, 0]], device=dev), 32, walk_length=4, context_size=3, num_nodes=2)
    ok = torch.tensor([[0, 1, 0]], device=dev)
    with pytest.raises(IndexError):
        m.loss(torch.tensor([[0, 1, 2]], device=dev), ok)
    with pytest.raises(IndexError):
        m.loss(ok, torch.tensor([[0, -1, 1]], device=dev))


# ---- SparseAdam --------------------------------------------------------------------------------------------------------------
def test_sparse_adam_matches_torch(dev):
    from graphpope_amd import node2vec
    n, d, lr = 1000, 128, 0.01
    g = torch.Generator(device="cpu").manual_seed(0)
    p0 = torch.randn(n, d, generator=g).to(dev)
    refs = {}
    for dt in (torch.float32, torch.float64):
        p = p0.to(dt).clone().requires_grad_(True)
        refs[dt] = (p, torch.optim.SparseAdam([p], lr=lr))
    emb, grad = p0.clone(), torch.zeros(n, d, device=dev)
    touched = torch.zeros(n, dtype=torch.uint8, device=dev)
    m1, m2 = torch.zeros_like(emb), torch.zeros_like(emb)
    for step, share in enumerate((0.05, 0.5, 0.0), start=1):
        rows = torch.nonzero(torch.rand(n, generator=g) < share).flatten().to(dev)
        vals = (torch.randn(rows.numel(), d, generator=g) * 10.0 ** float(torch.randn((), generator=g))).to(dev)
        for dt, (p, opt) in refs.items():
            p.grad = torch.sparse_coo_tensor(rows[None], vals.to(dt), (n, d))
            opt.step()
        grad[rows] = vals
        touched[rows] = 1
        before = (emb.clone(), m1.clone(), m2.clone())
        node2vec.sparse_adam(emb, grad, touched, m1, m2, lr, 0.9, 0.999, 1e-8, step)
        assert not grad.any() and not touched.any()                              # the next step starts clean
        keep = torch.ones(n, dtype=torch.bool, device=dev)
        keep[rows] = False
        for now, was in zip((emb, m1, m2), before):                              # untouched rows: bitwise unchanged, moments included
            assert torch.equal(now[keep].view(torch.int32), was[keep].view(torch.int32))
        if share == 0.0:
            assert rows.numel() == 0 and all(torch.equal(now, was) for now, was in zip((emb, m1, m2), before))
        else:
            assert rows.numel() > 0 and not torch.equal(emb[rows], before[0][rows])
        st32, st64 = refs[torch.float32][1].state[refs[torch.float32][0]], refs[torch.float64][1].state[refs[torch.float64][0]]
        _assert_no_worse_than_torch(emb, refs[torch.float32][0].detach(), refs[torch.float64][0].detach(), f"step {step} parameters")
        _assert_no_worse_than_torch(m1, st32["exp_avg"], st64["exp_avg"], f"step {step} exp_avg")
        _assert_no_worse_than_torch(m2, st32["exp_avg_sq"], st64["exp_avg_sq"], f"step {step} exp_avg_sq")


# ---- training ----------------------------------------------------------------------------------------------------------------
def _community_graph(seed, n=512, communities=4):
    """label = v % 4.  For v in order: 8 targets with replacement from v's community, then 1 from the others; self-loops dropped, both
    directions added, duplicates removed."""
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


def _centroid_accuracy(table, n=512, communities=4):
    z = F.normalize(table.double().cpu(), dim=1)
    v = torch.arange(n)
    label, fit_half = v % communities, (v // communities) % 2 == 0
    centroids = torch.stack([z[fit_half & (label == c)].mean(0) for c in range(communities)])
    pred = (z[~fit_half] @ centroids.T).argmax(1)
    return float((pred == label[~fit_half]).double().mean())


@pytest.mark.parametrize("seed", [0, 1])
def test_training_learns_the_communities(dev, seed):
    from graphpope_amd.node2vec import Node2Vec
    torch.manual_seed(seed)
    m = Node2Vec(torch.as_tensor(_community_graph(seed), device=dev), 32, walk_length=10, context_size=5, walks_per_node=4,
                 num_negative_samples=1, num_nodes=512)
    with torch.no_grad():                                                        # the untrained table on the same sampler
        first = [float(m.loss(*m.sample(b, seed=1000 + i))) for i, b in enumerate(m._batches(64, False, None))]
    untrained, acc0 = float(np.mean(first)), _centroid_accuracy(m.embedding.weight.detach())
    losses = m.fit(epochs=8, batch_size=64, lr=0.05, seed=seed)
    acc = _centroid_accuracy(m.embedding.weight.detach())
    print(f"seed {seed}: untrained loss {untrained:.3f} accuracy {acc0:.3f}; epoch losses {[round(x, 3) for x in losses]}; accuracy {acc:.3f}")
    assert len(losses) == 8 and m.step_count == 64 and torch.isfinite(m.embedding.weight).all()
    assert not m.grad.any() and not m.touched.any()
    assert acc >= 0.95
    assert losses[-1] < 0.5 * untrained


# ---- command line and hand-over ----------------------------------------------------------------------------------------------
def test_generator_writes_the_table_attach_node2vec_loads(dev, tmp_path, monkeypatch):
    from graphpope_amd import generate_node2vec_embedding as gen, utils as gp
    n, f, k = 512, 12, 16
    ei = _community_graph(0)
    x = np.random.default_rng(1).random((n, f), dtype=np.float32)
    mask = np.ones(n, dtype=bool)
    np.savez(tmp_path / "pubmed.npz", x=x, y=np.arange(n) % 3, edge_index=ei, train_mask=mask, val_mask=mask, test_mask=mask)
    out = tmp_path / "pubmed_node2vec.pt"
    gen.main(["--dataset", "pubmed", "--epochs", "0", "--data_dir", str(tmp_path), "--out", str(out)])
    table = torch.load(out)
    assert isinstance(table, torch.Tensor) and not table.is_cuda and table.dtype == torch.float32 and table.shape == (n, 128)
    assert not table.requires_grad
    torch.manual_seed(42)
    want = torch.nn.Embedding(n, 128).weight.detach()
    assert torch.equal(table.view(torch.int32), want.view(torch.int32))          # the reference's behaviour: the untrained table
    gen.main(["--dataset", "PubMed", "--epochs", "1", "--data_dir", str(tmp_path), "--out", str(out)])
    trained = torch.load(out)
    assert trained.shape == (n, 128) and trained.dtype == torch.float32 and torch.isfinite(trained).all()
    assert not torch.equal(trained, table)

    class Data:
        pass
    d = Data()
    d.x, d.edge_index, d.num_nodes = torch.as_tensor(x), torch.as_tensor(ei), n
    monkeypatch.setattr(gp, "NODE2VEC_DIR", str(tmp_path))
    gp.clear_cache()
    np.random.seed(42)
    feats = gp.Graphpope(d, "pubmed", embedding_space="node2vec", sampling_method="stochastic", num_anchor_nodes=k,
                         distance_function="euclidean")
    gp.clear_cache()
    assert feats.shape == (n, f + k) and feats.dtype == torch.float32 and torch.equal(feats[:, :f], d.x)
    emb = feats[:, f:]
    assert torch.isfinite(emb).all() and float(emb.min()) >= 0.0 and float(emb.max()) <= 1.0 + 1e-6 and float(emb.std()) > 0.0
