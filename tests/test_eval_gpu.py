"""Device-resident evaluation: sage_eval_metrics (sage.EvalMetrics) against NumPy float64, and the replayed forward-only step
(train.SageEvalStep) against the eager evaluation loop of graphpope_amd.main -- main.py:216-217, 224-241."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MS = (1, 63, 65, 257, 1550)          # rows per wave below and above one, more rows than the grid has waves (64 blocks x 4)


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


def _reference(logits: np.ndarray, y: np.ndarray, ignore_index=-100):
    """(float64 loss sum, correct, rows) over the rows whose label is inside [0, C) and not ignore_index."""
    x = logits.astype(np.float64)
    keep = (y >= 0) & (y < x.shape[1]) & (y != ignore_index)
    x, y = x[keep], y[keep]
    if x.shape[0] == 0:
        return 0.0, 0, 0
    mx = x.max(axis=1)
    with np.errstate(invalid="ignore"):
        lse = mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))
    loss = lse - x[np.arange(x.shape[0]), y]
    return float(loss.sum()), int((np.argmax(logits[keep], axis=1) == y).sum()), int(x.shape[0])


def _raw(metrics):
    """The three device words as (float64 loss sum, correct, rows)."""
    w = metrics.acc.cpu().numpy()
    return float(w[:1].view(np.float64)[0]), int(w[1]), int(w[2])


def _run(dev, logits: np.ndarray, y: np.ndarray, metrics=None):
    from graphpope_amd.sage import EvalMetrics
    metrics = metrics or EvalMetrics(dev)
    metrics.update(torch.as_tensor(logits, device=dev), torch.as_tensor(y, device=dev))
    return metrics


@pytest.mark.parametrize("c", [1, 3, 7, 64, 65, 256, 512, 513, 700])
def test_metrics_kernel_equals_numpy(dev, c):
    """Standard-normal logits: counts exact, mean loss within 1e-6 relative of float64 (the gate of tests/test_epilogue_gpu.py)."""
    rng = np.random.RandomState(1000 + c)
    for m in MS:
        logits = rng.randn(m, c).astype(np.float32)
        y = rng.randint(0, c, m).astype(np.int64)
        y[1::3] = np.argmax(logits[1::3], axis=1)                # a third of the rows are hits whatever C is
        want_loss, want_correct, want_rows = _reference(logits, y)
        metrics = _run(dev, logits, y)
        got_loss, got_correct, got_rows = _raw(metrics)
        print(f"C={c} M={m}: loss sum {got_loss!r} vs {want_loss!r}, correct {got_correct} vs {want_correct}")
        assert (got_correct, got_rows) == (want_correct, want_rows) and want_rows == m
        assert abs(got_loss / m - want_loss / m) <= 1e-6 * abs(want_loss / m)
        mean, acc, rows = metrics.read()
        assert rows == m and acc == want_correct / m and mean == got_loss / m


def test_metrics_kernel_on_large_logits_is_as_good_as_torch(dev):
    """Logits scaled by 80 (the maximum subtraction matters): the error of the kernel's loss sum against float64 is at most twice
    the error of torch's own float32 F.cross_entropy(reduction='sum') on the same device."""
    rng = np.random.RandomState(7)
    m, c = 1550, 256
    logits = (80.0 * rng.randn(m, c)).astype(np.float32)
    y = rng.randint(0, c, m).astype(np.int64)
    want_loss, want_correct, _ = _reference(logits, y)
    got_loss, got_correct, got_rows = _raw(_run(dev, logits, y))
    torch_loss = float(F.cross_entropy(torch.as_tensor(logits, device=dev), torch.as_tensor(y, device=dev), reduction="sum").double())
    print(f"float64 {want_loss!r}: kernel error {abs(got_loss - want_loss):.6g}, torch error {abs(torch_loss - want_loss):.6g}")
    assert (got_correct, got_rows) == (want_correct, m)
    assert abs(got_loss - want_loss) <= 2.0 * abs(torch_loss - want_loss)


def test_argmax_ties_go_to_the_first_column(dev):
    """numpy.argmax's rule where a shuffle tree's lane order would disagree.  Every row is run twice: labelled with the first of
    its equal maxima (a hit) and with the other one (a miss)."""
    rows = []                                                     # (C, first, other)

    def tie(c, a, b):
        r = np.random.RandomState(c * 1000 + a).randn(c).astype(np.float32)
        r[[a, b]] = 9.0
        rows.append((r, min(a, b), max(a, b)))

    tie(128, 3, 67)                                               # one lane, k = 0 and k = 1
    tie(128, 70, 5)                                               # lanes 6 and 5: the later column sits in the earlier lane's k = 1
    tie(65, 10, 64)                                               # the last, partial group of C = 65 against another lane
    tie(65, 0, 64)                                                # ... and against its own lane
    tie(700, 650, 13)                                             # the looped form
    for c in (65, 128, 700):
        rows.append((np.full(c, 0.25, dtype=np.float32), 0, c - 1))     # all equal
    for r, first, other in rows:
        assert int(np.argmax(r)) == first
        block = np.tile(r, (5, 1))                                # more than one row per wave iteration
        for label, hits in ((first, 5), (other, 0)):
            _, correct, n = _raw(_run(dev, block, np.full(5, label, dtype=np.int64)))
            assert (correct, n) == (hits, 5), (r.shape[0], first, other, label)


@pytest.mark.parametrize("c", [65, 600])
def test_a_nan_is_the_maximum_and_poisons_the_loss(dev, c):
    rng = np.random.RandomState(c)
    logits = rng.randn(9, c).astype(np.float32)
    logits[2, 40], logits[2, 9], logits[2, 50] = np.nan, np.nan, 100.0          # the first NaN wins, a larger number does not
    logits[5, 64] = np.nan                                                     # lane 0's second column
    y = np.zeros(9, dtype=np.int64)
    y[2], y[5] = 9, 0
    assert np.argmax(logits[2]) == 9 and np.argmax(logits[5]) == 64
    y[7] = np.argmax(logits[7])
    _, want_correct, _ = _reference(logits, y)
    got_loss, got_correct, n = _raw(_run(dev, logits, y))
    assert np.isnan(got_loss) and (got_correct, n) == (want_correct, 9) and want_correct >= 2
    y[2] = 40                                                                  # the second NaN is not the argmax
    assert _raw(_run(dev, logits, y))[1] == want_correct - 1


@pytest.mark.parametrize("c", [7, 600])
def test_ignored_and_out_of_range_labels_are_left_out(dev, c):
    from graphpope_amd.sage import bad_label_flag
    rng = np.random.RandomState(3)
    logits = rng.randn(40, c).astype(np.float32)
    y = rng.randint(0, c, 40).astype(np.int64)
    flag = bad_label_flag(dev)
    flag.zero_()
    y[[1, 17, 39]] = -100
    want = _reference(logits, y)
    got = _raw(_run(dev, logits, y))
    assert got[1:] == want[1:] and want[2] == 37 and abs(got[0] - want[0]) <= 1e-6 * want[0]
    assert int(flag.item()) == 0                                  # ignore_index alone does not set the flag
    y[[0, 8, 30]] = (-1, c, c + 5)
    want = _reference(logits, y)
    got = _raw(_run(dev, logits, y))
    assert got[1:] == want[1:] and want[2] == 34 and abs(got[0] - want[0]) <= 1e-6 * want[0]
    assert int(flag.item()) == 1
    flag.zero_()


def test_updates_accumulate_and_reset_zeroes(dev):
    from graphpope_amd.sage import EvalMetrics
    rng = np.random.RandomState(5)
    metrics = EvalMetrics(dev)
    total = np.zeros(3)
    for m, c in ((257, 7), (63, 65), (100, 600)):
        logits = rng.randn(m, c).astype(np.float32)
        y = rng.randint(0, c, m).astype(np.int64)
        y[::2] = np.argmax(logits[::2], axis=1)
        total += _reference(logits, y)
        _run(dev, logits, y, metrics)
    got = _raw(metrics)
    assert got[1:] == (int(total[1]), int(total[2])) and abs(got[0] - total[0]) <= 1e-6 * total[0]
    metrics.reset()
    assert metrics.acc.cpu().tolist() == [0, 0, 0] and metrics.read()[2] == 0


# ---- SageEvalStep against the eager loop -------------------------------------------------------------------------------------

BATCH, ORDER_LEN, SAMPLE_SEED = 64, 5 * 64 + 17, (3 << 20) + (2 << 10)


@pytest.fixture(scope="module")
def graph(dev):
    from graphpope_amd import engine, synth
    ei = synth.powerlaw_graph(6000, 40000, seed=7, alpha=0.9, shift=0.8)
    csr = engine.build_csr(torch.as_tensor(ei, device=dev), 6000)
    labels = torch.randint(0, 5, (6000,), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    order = torch.randperm(6000, device=dev, generator=torch.Generator(device=dev).manual_seed(3))[:ORDER_LEN].contiguous()
    return dev, csr, labels, order


def _trained_model(dev, csr, labels, sizes, c_in, hidden):
    """(model, feats, sampler) with BatchNorm running statistics made non-trivial by one training step."""
    from graphpope_amd.optim import Adam
    from graphpope_amd.sage import SAGE, IndexedFeatures, cross_entropy
    from graphpope_amd.sampler import NeighborSampler
    feats = torch.randn(6000, c_in, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    sampler = NeighborSampler(csr.rowptr, csr.col, 6000, sizes)
    torch.manual_seed(0)
    model = SAGE(c_in, 5, hidden, 3).to(dev)
    opt = Adam(model.parameters(), lr=0.01)
    seeds = torch.arange(1000, 1256, device=dev)
    n_id, adjs = sampler.sample(seeds, seed=1)
    model.train()
    cross_entropy(model(IndexedFeatures(feats, n_id), adjs), labels[seeds].contiguous()).backward()
    opt.step()
    return model, feats, sampler, opt


def _eager_batches(model, feats, sampler, labels, order, sample_seed, batch=BATCH):
    """What graphpope_amd.main's eager evaluation loop computes: per batch (n_id, y, logits)."""
    from graphpope_amd.sage import IndexedFeatures
    was = model.training
    model.eval()
    out = []
    with torch.no_grad():
        for b, lo in enumerate(range(0, order.numel(), batch)):
            seeds = order[lo:lo + batch].contiguous()
            n_id, adjs = sampler.sample(seeds, seed=sample_seed + b)
            out.append((n_id, labels.index_select(0, seeds), model(IndexedFeatures(feats, n_id), adjs)))
    model.train(was)
    return out


@pytest.fixture(scope="module", params=[((25, 10), 40, 48), ((5, 3), 37, 30)], ids=["two_hops", "odd_widths"])
def case(graph, request):
    dev, csr, labels, order = graph
    sizes, c_in, hidden = request.param
    model, feats, sampler, _ = _trained_model(dev, csr, labels, sizes, c_in, hidden)
    refs = {n: _eager_batches(model, feats, sampler, labels, order[:n].contiguous(), SAMPLE_SEED) for n in (ORDER_LEN, 3 * BATCH, 17)}
    return model, feats, sampler, refs


def _recorded_pass(ev, order, labels, sample_seed):
    """run_pass with every batch's (n_id, y, logits) copied on the way: full batches through ev.step, then the tail."""
    seen, step = [], ev.step

    def recording_step():
        logits = step()
        seen.append((ev.batch.n_id[: int(ev.batch.dims[-1][1])].clone(), ev.y.clone(), logits.clone()))
        return logits

    ev.step = recording_step
    ev.tail_logits = None
    try:
        loss, acc = ev.run_pass(order, labels, sample_seed)
    finally:
        del ev.step
    if ev.tail_logits is not None:
        tail = order[len(seen) * ev.batch.n_seeds:]
        seen.append((None, labels.index_select(0, tail), ev.tail_logits.clone()))
    return loss, acc, seen


def _check_pass(loss, acc, rows, seen, want_rows):
    """run_pass's figures against NumPy on the step's own logits: the count exactly, the loss within 1e-6 relative."""
    total = np.zeros(3)
    for _, y, logits in seen:
        total += _reference(logits.cpu().numpy(), y.cpu().numpy())
    assert rows == want_rows == int(total[2])
    assert acc == int(total[1]) / rows
    assert abs(loss - total[0] / rows) <= 1e-6 * abs(total[0] / rows)


@pytest.mark.parametrize("n", [ORDER_LEN, 3 * BATCH, 17], ids=["five_and_a_tail", "no_tail", "tail_only"])
@pytest.mark.parametrize("use_graph", [True, False], ids=["replayed", "eager_body"])
def test_eval_step_equals_the_eager_loop(graph, case, use_graph, n):
    """Batch b of the pass is the batch sampler.sample(order[b * 64 : ...], sample_seed + b) draws, its logits those of model.eval() on
    it (tolerance of test_device_extent_layers_equal_the_host_sized_ones), its node list and labels equal exactly."""
    from graphpope_amd.train import SageEvalStep
    dev, _, labels, order = graph
    model, feats, sampler, refs = case
    order = order[:n].contiguous()
    ev = SageEvalStep(model, feats, BATCH, sampler, graph=use_graph)
    model.train()
    for _ in range(2):                                            # the second pass replays from its first batch
        loss, acc, seen = _recorded_pass(ev, order, labels, SAMPLE_SEED)
        assert model.training
        want = refs[n]
        assert len(seen) == len(want) == (n + BATCH - 1) // BATCH
        for (n_id, y, logits), (w_id, w_y, w_logits) in zip(seen, want):
            assert n_id is None or torch.equal(n_id, w_id)
            assert torch.equal(y[: w_y.numel()], w_y)
            assert logits.shape == w_logits.shape and torch.allclose(logits, w_logits, rtol=1e-5, atol=1e-6)
        _check_pass(loss, acc, ev.rows, seen, n)
    assert (ev._graph is not None) == (use_graph and n >= 3 * BATCH)


def _snapshot(model, opt, trainer):
    tensors = [p for p in model.parameters()] + [p.grad for p in model.parameters() if p.grad is not None]
    for bn in model.bns:
        tensors += [bn.running_mean, bn.running_var, bn.num_batches_tracked]
    for st in opt.state.values():
        tensors += [v for v in st.values() if torch.is_tensor(v)]
    tensors.append(trainer.state.words)
    return tensors, [t.detach().clone() for t in tensors]


def _train_setup(graph, seed=11):
    from graphpope_amd.optim import Adam
    from graphpope_amd.sage import SAGE
    from graphpope_amd.sampler import NeighborSampler
    from graphpope_amd.train import SageTrainStep
    dev, csr, labels, _ = graph
    feats = torch.randn(6000, 40, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    sampler = NeighborSampler(csr.rowptr, csr.col, 6000, (25, 10))
    torch.manual_seed(0)
    model = SAGE(40, 5, 48, 3).to(dev)
    opt = Adam(model.parameters(), lr=0.01, max_grad_norm=0.5)
    trainer = SageTrainStep(model, opt, feats, 128, sampler=sampler, graph=True, seed=seed)
    perm = torch.randperm(6000, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    batches = [perm[i * 128:(i + 1) * 128].contiguous() for i in range(6)]
    return model, opt, trainer, feats, sampler, batches


def test_an_eval_pass_disturbs_nothing(graph):
    from graphpope_amd.train import SageEvalStep
    dev, _, labels, order = graph
    model, opt, trainer, feats, sampler, batches = _train_setup(graph)
    for sd in batches[:3]:
        trainer.step(sd, labels[sd].contiguous())
    tensors, before = _snapshot(model, opt, trainer)
    assert len(before) > 20 and any(t.dtype == torch.float32 and t.numel() > 100 for t in before)
    seed_word = model.dropout_seed_dev
    ev = SageEvalStep(model, feats, BATCH, sampler)
    for training in (True, False):
        model.train(training)
        ev.run_pass(order, labels, SAMPLE_SEED)
        assert model.training == training
    assert ev._graph is not None
    after_tensors, _ = _snapshot(model, opt, trainer)
    assert len(after_tensors) == len(tensors) and all(a is b for a, b in zip(after_tensors, tensors))
    for t, b in zip(tensors, before):
        assert torch.equal(t.detach().reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))
    assert model.dropout_seed_dev is seed_word or model.dropout_seed_dev.data_ptr() == seed_word.data_ptr()


def test_eval_passes_between_replayed_training_steps(graph):
    """train replay, eval pass, train replay, eval pass: the second pass equals the eager evaluation with the updated weights (the
    replay reads live weights), and the training losses are those of the same steps without evaluation in between."""
    from graphpope_amd.train import SageEvalStep
    dev, _, labels, order = graph
    runs = []
    for with_eval in (False, True):
        model, opt, trainer, feats, sampler, batches = _train_setup(graph)
        for sd in batches[:3]:                                    # two eager calls and the capture
            trainer.step(sd, labels[sd].contiguous())
        assert trainer._graph is not None
        ev = SageEvalStep(model, feats, BATCH, sampler) if with_eval else None
        losses, passes = [], []
        for sd in batches[3:5]:
            losses.append(trainer.step(sd, labels[sd].contiguous()).item())
            if with_eval:
                passes.append(_recorded_pass(ev, order, labels, SAMPLE_SEED))
        runs.append(losses)
    assert np.allclose(runs[0], runs[1], rtol=1e-4)
    assert ev._graph is not None
    want = _eager_batches(model, feats, sampler, labels, order, SAMPLE_SEED)
    (_, _, first), (loss, acc, second) = passes
    assert len(second) == len(want) == 6
    for (n_id, y, logits), (w_id, w_y, w_logits) in zip(second, want):
        assert n_id is None or torch.equal(n_id, w_id)
        assert torch.allclose(logits, w_logits, rtol=1e-5, atol=1e-6)
    assert not torch.allclose(first[0][2], second[0][2], rtol=1e-3, atol=1e-4)      # the training step in between moved the weights
    _check_pass(loss, acc, ev.rows, second, ORDER_LEN)


def test_run_epoch_with_the_replayed_step_agrees_with_the_eager_path(graph, case, monkeypatch):
    """graphpope_amd.main._run_epoch over a validation split: the default (SageEvalStep) against GRAPHPOPE_EVAL_STEP=eager."""
    from graphpope_amd import main as cli
    dev, _, labels, order = graph
    model, feats, sampler, _ = case
    args = argparse.Namespace(batch_size=BATCH, seed=5)
    epoch = 2
    monkeypatch.delenv("GRAPHPOPE_EVAL_STEP", raising=False)
    ev = cli._make_evaluator(model, feats, BATCH, sampler, order.numel())
    assert ev is not None and cli._make_evaluator(model, feats, BATCH, sampler, BATCH - 1) is None
    got = [cli._run_epoch(model, feats, labels, sampler, order, args, None, epoch, evaluator=ev) for _ in range(2)]
    assert ev._graph is not None and ev.rows == order.numel()
    monkeypatch.setenv("GRAPHPOPE_EVAL_STEP", "eager")
    assert cli._make_evaluator(model, feats, BATCH, sampler, order.numel()) is None
    want_loss, want_acc = cli._run_epoch(model, feats, labels, sampler, order, args, None, epoch, evaluator=None)
    # rows of the eager logits whose two largest entries are closer than the two paths' logits may differ: only those may flip
    close = 0
    for _, _, logits in _eager_batches(model, feats, sampler, labels, order, (args.seed << 20) + (epoch << 10)):
        top = logits.double().topk(2, dim=1).values
        close += int(((top[:, 0] - top[:, 1]) < 1e-5 * top[:, 0].abs() + 1e-6).sum())
    print(f"eager {want_loss!r} {want_acc!r}; replayed {got!r}; rows with a top-two gap inside the tolerance: {close}")
    assert close <= 0.01 * order.numel()
    for loss, acc in got:
        assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)
        assert abs(acc - want_acc) * order.numel() <= close + 1e-9
