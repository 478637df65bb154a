"""Gradient-norm clipping inside the one-launch Adam step (graphpope_amd.optim.Adam(max_grad_norm=...): sage_grad_sqnorm +
sage_adam_step_clip) against what the reference runs, torch.nn.utils.clip_grad_norm_(parameters, 0.5) in front of
torch.optim.Adam (main.py:285-290 gradient_clip_val=0.5, main.py:244).

Parity is judged against the same torch code on float64 copies: the error of this optimiser against float64, relative to the
largest float64 magnitude of the tensor, may be at most twice the error of torch's float32 run, plus 1e-6 (the bound
test_optim_gpu.py uses for the same formulas; the factor 2 covers one differing rounding of the coefficient -- torch forms it as
reciprocal * max_norm from a float32 norm of float32 norms, here it is one division from a float64 sum)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(256, 756), (256,), (7, 256), (5000,), (3, 3, 3), (1,), (4097,)] + [(i + 1, 3) for i in range(20)]     # 27 > ADAM_MAX_TENSORS = 24


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


def _rel_err(a, ref64):
    return float((a.double() - ref64).abs().max()) / max(float(ref64.abs().max()), 1e-300)


def _assert_no_worse_than_torch(mine, ref32, ref64, what):
    e_mine, e_torch = _rel_err(mine, ref64), _rel_err(ref32, ref64)
    print(f"{what}: this {e_mine:.3e} torch float32 {e_torch:.3e}")
    assert e_mine <= 2.0 * e_torch + 1e-6, (what, e_mine, e_torch)


def _expected_coef(norm32, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in IEEE float32, on the host."""
    c = np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else c


def _check_norm_and_coef(opt, grads, max_norm):
    norm64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
    got = np.float32(opt.grad_norm.item())
    print(f"grad_norm {got!r} float64 {norm64!r} coef {opt.clip_coef.item()!r}")
    assert abs(float(got) - norm64) <= 2.0 ** -23 * norm64
    coef = np.float32(opt.clip_coef.item())
    assert coef.view(np.uint32) == _expected_coef(got, max_norm).view(np.uint32)
    return float(coef)


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_matches_torch_clip_and_adam_judged_against_float64(weight_decay, dev):
    from graphpope_amd.optim import Adam
    torch.manual_seed(0)
    max_norm = 0.5
    p32 = [torch.randn(s, device=dev).requires_grad_(True) for s in SHAPES]
    p64 = [p.detach().double().requires_grad_(True) for p in p32]
    mine_p = [p.detach().clone().requires_grad_(True) for p in p32]
    unused = torch.randn(10, device=dev, requires_grad=True)
    unused_before = unused.detach().clone()
    ref32 = torch.optim.Adam(p32, lr=0.01, weight_decay=weight_decay)
    ref64 = torch.optim.Adam(p64, lr=0.01, weight_decay=weight_decay)
    mine = Adam(mine_p + [unused], lr=0.01, weight_decay=weight_decay, max_grad_norm=max_norm)
    assert "max_grad_norm" not in mine.defaults and all("max_grad_norm" not in g for g in mine.param_groups)
    scales = [1e-4, 1.0, 1e-5, 10.0, 1e-4, 0.1]        # the norm of all gradients is ~450 x the scale: three steps clip, three do not
    coefs = []
    for step, scale in enumerate(scales):
        grads = [torch.randn_like(p) * scale for p in p32]
        for a, b, c, g in zip(p32, p64, mine_p, grads):
            a.grad, b.grad, c.grad = g.clone(), g.double(), g.clone()
        torch.nn.utils.clip_grad_norm_(p32, max_norm)
        torch.nn.utils.clip_grad_norm_(p64, max_norm)
        ref32.step(); ref64.step(); mine.step()
        coefs.append(_check_norm_and_coef(mine, grads, max_norm))
        for c, g in zip(mine_p, grads):
            assert torch.equal(c.grad, g)                                  # p.grad is not modified (torch scaled a.grad in place)
        for i, (a, b, c) in enumerate(zip(p32, p64, mine_p)):
            _assert_no_worse_than_torch(c.detach(), a.detach(), b.detach(), f"step {step} param {i}")
    assert sum(c < 1.0 for c in coefs) >= 2 and sum(c == 1.0 for c in coefs) >= 2, coefs
    for i, (a, b, c) in enumerate(zip(p32, p64, mine_p)):
        for key in ("exp_avg", "exp_avg_sq"):
            _assert_no_worse_than_torch(mine.state[c][key], ref32.state[a][key], ref64.state[b][key], f"{key} {i}")
        assert mine.state[c]["step"] == 6
    assert torch.equal(unused.detach(), unused_before) and (unused not in mine.state or not mine.state[unused])


def test_two_param_groups_share_one_global_norm(dev):
    from graphpope_amd.optim import Adam
    torch.manual_seed(1)
    max_norm = 1.0
    shapes_a, shapes_b = [(300, 40), (40,)], [(5000,), (17,)]
    a32 = [torch.randn(s, device=dev).requires_grad_(True) for s in shapes_a]
    b32 = [torch.randn(s, device=dev).requires_grad_(True) for s in shapes_b]
    a64, b64 = [p.detach().double().requires_grad_(True) for p in a32], [p.detach().double().requires_grad_(True) for p in b32]
    am, bm = [p.detach().clone().requires_grad_(True) for p in a32], [p.detach().clone().requires_grad_(True) for p in b32]
    no_grad = torch.randn(50, device=dev, requires_grad=True)               # in a group, never given a gradient
    groups = lambda a, b: [{"params": a, "lr": 0.01}, {"params": b, "lr": 0.001}]
    ref32, ref64 = torch.optim.Adam(groups(a32, b32)), torch.optim.Adam(groups(a64, b64))
    mine = Adam(groups(am, bm + [no_grad]), max_grad_norm=max_norm)
    for step in range(4):
        grads = [torch.randn_like(p) * (0.02 if i < len(a32) else 0.5) for i, p in enumerate(a32 + b32)]   # group b carries the norm
        for p, q, r, g in zip(a32 + b32, a64 + b64, am + bm, grads):
            p.grad, q.grad, r.grad = g.clone(), g.double(), g.clone()
        torch.nn.utils.clip_grad_norm_(a32 + b32, max_norm)
        torch.nn.utils.clip_grad_norm_(a64 + b64, max_norm)
        ref32.step(); ref64.step(); mine.step()
        coef = _check_norm_and_coef(mine, grads, max_norm)                  # the norm over BOTH groups; no_grad does not enter
        assert coef < 0.1                                                   # group a alone (norm ~2.2) would get ~0.45
    for i, (p, q, r) in enumerate(zip(a32 + b32, a64 + b64, am + bm)):
        _assert_no_worse_than_torch(r.detach(), p.detach(), q.detach(), f"param {i}")
        for key in ("exp_avg", "exp_avg_sq"):
            _assert_no_worse_than_torch(mine.state[r][key], ref32.state[p][key], ref64.state[q][key], f"{key} {i}")
    assert no_grad not in mine.state or not mine.state[no_grad]


def _run_clipped(dev, seed, steps=4, **kw):
    from graphpope_amd.optim import Adam
    g = torch.Generator(device=dev).manual_seed(seed)
    ps = [torch.randn(s, device=dev, generator=g).requires_grad_(True) for s in SHAPES]
    opt = Adam(ps, lr=0.01, weight_decay=0.01, **kw)
    for step in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev, generator=g) * (1e-4 if step % 2 else 1.0)
        opt.step()
    return [p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps for k in ("exp_avg", "exp_avg_sq")]


def test_same_inputs_give_the_same_bits(dev):
    a, b = _run_clipped(dev, 5, max_grad_norm=0.5), _run_clipped(dev, 5, max_grad_norm=0.5)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_none_is_the_plain_optimiser(dev):
    a, b = _run_clipped(dev, 6, max_grad_norm=None), _run_clipped(dev, 6)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = _run_clipped(dev, 6, max_grad_norm=0.5)
    assert not all(torch.equal(x, y) for x, y in zip(a, c))                 # and a value is not


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_non_finite_gradients_poison_what_torch_poisons(bad, dev):
    """error_if_nonfinite=False: an inf makes the norm inf and the coefficient 0 (0 * inf = nan in that one element), a nan makes
    the coefficient nan (every element)."""
    from graphpope_amd.optim import Adam
    torch.manual_seed(2)
    shapes = [(300, 40), (40,), (5000,)]
    ref_p = [torch.randn(s, device=dev).requires_grad_(True) for s in shapes]
    my_p = [p.detach().clone().requires_grad_(True) for p in ref_p]
    ref, mine = torch.optim.Adam(ref_p, lr=0.01), Adam(my_p, lr=0.01, max_grad_norm=0.5)
    for step in range(2):
        for a, b in zip(ref_p, my_p):
            g = torch.randn_like(a)
            if step == 1 and a.dim() == 2:
                g[17, 3] = bad
            a.grad, b.grad = g.clone(), g.clone()
        torch.nn.utils.clip_grad_norm_(ref_p, 0.5)
        ref.step(); mine.step()
        for a, b in zip(ref_p, my_p):
            assert torch.equal(torch.isnan(a.detach()), torch.isnan(b.detach())), step
    n_nan = sum(int(torch.isnan(b.detach()).sum()) for b in my_p)
    assert n_nan == (1 if bad == float("inf") else sum(p.numel() for p in my_p))
    assert torch.isinf(mine.grad_norm) if bad == float("inf") else torch.isnan(mine.grad_norm)


def test_device_step_word_and_folded_loss_with_clipping(dev):
    """use_device_step + fold_loss (cross_entropy(loss_in=opt)) through the clipping entry point: the parameters of the host step
    count without a folded loss (test_adam_device_step_matches_the_host_step's tolerance) and the loss F.cross_entropy gives
    (test_cross_entropy_finished_by_the_optimisers_launch's)."""
    from graphpope_amd.optim import Adam
    from graphpope_amd.sage import cross_entropy
    torch.manual_seed(3)
    n, c = 1550, 64
    w = torch.randn(c, c, device=dev) * 0.1
    folded, plain, ref = torch.nn.Parameter(w.clone()), torch.nn.Parameter(w.clone()), torch.nn.Parameter(w.clone())
    opt, popt = Adam([folded], lr=1e-2, max_grad_norm=0.5), Adam([plain], lr=1e-2, max_grad_norm=0.5)
    word = torch.ones(1, dtype=torch.int64, device=dev)
    opt.use_device_step(word)
    coefs = []
    for rep in range(4):
        x = torch.randn(n, c, device=dev) * (2 if rep % 2 else 0.05)
        y = torch.randint(0, c, (n,), device=dev)
        y[::6] = -100
        opt.zero_grad(set_to_none=True)
        ref.data.copy_(folded.data)
        ref.grad = None
        loss = cross_entropy(x @ folded, y, unit_upstream=True, loss_in=opt)
        loss.backward()
        want = F.cross_entropy(x @ ref, y)
        plain.grad = folded.grad.clone()
        opt.step(); popt.step()
        word += 1
        assert abs(float(loss.detach()) - float(want.detach())) <= 1e-6 * max(1.0, abs(float(want.detach()))), rep
        assert torch.allclose(folded.detach(), plain.detach(), rtol=1e-6, atol=1e-7), rep
        assert torch.equal(opt.clip_coef, popt.clip_coef)
        coefs.append(float(opt.clip_coef))
    assert min(coefs) < 1.0, coefs


# ---- the whole training step: fixtures and shapes of tests/test_train_gpu.py::test_replayed_step_equals_the_eager_step ----
@pytest.fixture(scope="module")
def graph():
    from graphpope_amd import engine, synth
    dev = engine.require_gpu()
    ei = synth.powerlaw_graph(6000, 40000, seed=7, alpha=0.9, shift=0.8)
    csr = engine.build_csr(torch.as_tensor(ei, device=dev), 6000)
    return dev, ei, csr


def _model(dev, c_in=40, hidden=48, layers=3):
    from graphpope_amd.sage import SAGE
    torch.manual_seed(0)
    return SAGE(c_in, 5, hidden, layers).to(dev)


@pytest.mark.parametrize("with_sampler", [True, False], ids=["sampler_in_graph", "presampled_pool"])
def test_step_with_the_optimisers_clip_replayed_eager_and_torch_clip(graph, with_sampler):
    """SageTrainStep over Adam(max_grad_norm=0.5), clip=None: replayed against eager, and both against SageTrainStep(clip=0.5)
    (torch's clip_grad_norm_) over the plain optimiser with the same seeds -- same losses, same parameters after 8 steps, to
    float-atomic noise."""
    from graphpope_amd.optim import Adam
    from graphpope_amd.sampler import DeviceBatch, NeighborSampler
    from graphpope_amd.train import SageTrainStep
    dev, _, csr = graph
    feats = torch.randn(6000, 40, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    labels = torch.randint(0, 5, (6000,), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    sampler = NeighborSampler(csr.rowptr, csr.col, 6000, (25, 10))
    perm = torch.randperm(6000, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    pool = []
    if not with_sampler:
        for i in range(4):
            sd = perm[i * 256:(i + 1) * 256].contiguous()
            n_id, adjs = sampler.sample(sd, seed=i)
            db = DeviceBatch(256, (25, 10), dev)
            db.load(n_id, adjs)
            pool.append((db, labels[sd].contiguous()))
    runs = []
    for use_graph, in_optimiser in ((False, True), (True, True), (False, False)):
        m = _model(dev)
        opt = Adam(m.parameters(), lr=0.01, max_grad_norm=0.5 if in_optimiser else None)
        st = SageTrainStep(m, opt, feats, 256, (25, 10), sampler=sampler if with_sampler else None, clip=None if in_optimiser else 0.5,
                           graph=use_graph, seed=11)
        losses, coefs = [], []
        for i in range(8):
            if with_sampler:
                sd = perm[(i % 6) * 256:(i % 6 + 1) * 256].contiguous()
                losses.append(st.step(sd, labels[sd].contiguous()).item())
            else:
                db, yb = pool[i % 4]
                st.load_batch(db, yb)
                losses.append(st.run().item())
            if in_optimiser:
                coefs.append(float(opt.clip_coef))
        runs.append((losses, [p.detach().clone() for p in m.parameters()], int(st.state.adam_step.item()),
                     opt.state_dict()["state"][0]["step"].item(), [bn.num_batches_tracked.item() for bn in m.bns[:1]], coefs))
    print("losses", [r[0] for r in runs], "coefficients", [r[5] for r in runs])
    for _, _, s, h, nb, _ in runs:
        assert s == 9 and h == 8.0 and nb == [8]
    eager, replayed, torch_clip = runs
    assert min(eager[5]) < 1.0 and min(replayed[5]) < 1.0                   # the clip did bite
    assert np.allclose(eager[5], replayed[5], rtol=1e-4)
    for other in (replayed, torch_clip):
        assert np.allclose(eager[0], other[0], rtol=1e-4) and other[0][-1] < other[0][0]
        for a, c in zip(eager[1], other[1]):
            assert float((a - c).norm()) <= 0.1 * float(a.norm()) + 1e-6


def test_two_clips_are_refused(graph):
    from graphpope_amd.optim import Adam
    from graphpope_amd.train import SageTrainStep
    dev = graph[0]
    m = _model(dev)
    feats = torch.zeros(6000, 40, device=dev)
    with pytest.raises(ValueError, match="twice"):
        SageTrainStep(m, Adam(m.parameters(), lr=0.01, max_grad_norm=0.5), feats, 256, (25, 10), clip=0.5)
    with pytest.raises(ValueError):
        Adam(m.parameters(), max_grad_norm=-1.0)
    SageTrainStep(m, Adam(m.parameters(), lr=0.01, max_grad_norm=0.5), feats, 256, (25, 10), clip=None)
