"""SAGEConv(normalize=True) and the models built from it on the GPU, through tests/sage_normalize_cases.py: one conv (direct and behind
IndexedFeatures, with and without bias) against the float64 dense formulation; the two-layer model's loss and every gradient against
the float64 model; conv + BatchNorm at a shape whose plain projection hands over statistics and takes its bias gradient from BatchNorm --
a normalising conv does neither; SAGE.inference against eval-mode forward; replayed training and evaluation steps against eager ones; and
normalize=False against the two-argument constructor, bit for bit."""
import numpy as np
import pytest
import torch

import sage_model_cases as mc
import sage_normalize_cases as cases
from workspace import dev, lib  # noqa: F401  (the fixtures live in the helper module)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    """A fault is sticky: every later call in the process would fail the same way.  The run ends at the test that met it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the GPU reported an error, nothing more is started: %s" % e, returncode=3)


@pytest.fixture
def lib_calls(monkeypatch):
    """The names of the library calls that enqueue work, in order (size and name queries are not recorded)."""
    from graphpope_amd import _lib
    real = _lib.load()
    calls = []

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("sage_") or name.endswith(("_bytes", "_size", "_name")):
                return fn
            return lambda *a: (calls.append(name), fn(*a))[1]
    monkeypatch.setattr(_lib, "load", Recorder)
    return calls


@pytest.fixture
def hidden(monkeypatch):
    """The output of every sage._bn_forward call, in order."""
    from graphpope_amd import sage
    real, seen = sage._bn_forward, []

    def wrapped(lib, x, gamma, beta, t, stats=None):
        out = real(lib, x, gamma, beta, t, stats)
        seen.append(out[0])
        return out
    monkeypatch.setattr(sage, "_bn_forward", wrapped)
    return seen


def _adj(dev, blk, n_src):
    from graphpope_amd import sage
    rowptr, col = blk
    return sage.SampledAdj(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), n_src)


def _conv(dev, t, normalize):
    from graphpope_amd import sage
    conv = sage.SAGEConv(t["w_l"].shape[1], t["w_l"].shape[0], normalize=normalize, bias="b_l" in t).to(dev)
    with torch.no_grad():
        conv.lin_l.weight.copy_(t["w_l"])
        conv.lin_r.weight.copy_(t["w_r"])
        if "b_l" in t:
            conv.lin_l.bias.copy_(t["b_l"])
    return conv


def _conv_grads(conv, x=None):
    got = {"grad:w_l": conv.lin_l.weight.grad.cpu(), "grad:w_r": conv.lin_r.weight.grad.cpu()}
    if conv.lin_l.bias is not None:
        got["grad:b_l"] = conv.lin_l.bias.grad.cpu()
    if x is not None:
        got["grad:x"] = x.grad.cpu()
    return got


# ------------------------------------------------------------------------------------------------ one conv

@pytest.mark.parametrize("way", ["direct", "indexed"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("c_out", cases.C_OUTS)
def test_conv_against_the_float64_dense_formulation(dev, lib_calls, c_out, bias, way):
    """70 sources, 33 destinations (row 4 without a neighbour), 12 -> c_out: the output and the gradients of x, W_l, b and W_r -- behind
    IndexedFeatures the feature matrix takes none."""
    from graphpope_amd import sage
    t, blk = cases.conv_inputs(c_out, bias)
    ref, limit = cases.conv_yardstick(t, blk)
    conv, adj = _conv(dev, t, True), _adj(dev, blk, cases.N_SRC)
    assert ("lin_l.bias" in conv.state_dict()) == bias
    if way == "direct":
        x = t["x"].to(dev).requires_grad_(True)
        out = conv((x, x[:cases.N_DST]), adj)
    else:
        n_id = torch.from_numpy(np.random.RandomState(3).permutation(200)[:cases.N_SRC]).to(dev)
        feats = torch.randn(200, cases.C_IN, generator=torch.Generator().manual_seed(1)).to(dev)
        feats[n_id] = t["x"].to(dev)
        x = None
        out = conv(sage.IndexedFeatures(feats, n_id), adj)
        ref, limit = ({k: v for k, v in d.items() if k != "grad:x"} for d in (ref, limit))
    (out * t["g"].to(dev)).sum().backward()
    got = dict(_conv_grads(conv, x), out=out.detach().cpu())
    cases.conv_check(got, ref, limit, "conv %d %s %s" % (c_out, "bias" if bias else "nobias", way))
    assert lib_calls == ["sage_conv_forward_indexed" if way == "indexed" else "sage_conv_forward", "sage_l2_normalize_forward",
                         "sage_l2_normalize_backward", "sage_conv_backward"]
    assert torch.allclose(out.detach().norm(dim=1), torch.ones(cases.N_DST, device=dev), atol=1e-5)


# ------------------------------------------------------------------------------------------------ the two-layer model

@pytest.mark.parametrize("p", [0.0, 0.5], ids=["dropout0", "dropout.5"])
def test_two_layer_model_against_the_float64_model(dev, lib_calls, hidden, p):
    """SAGE(12, 5, 16, 2, normalize=True) in training mode: logits, loss, the hidden activations, the running statistics and every
    parameter gradient.  The BatchNorm statistics are those of the normalised rows and the bias gradient is the conv's own: a model
    restated with either shortcut is outside these thresholds (test_sage_normalize_cpu.py), and neither hand-off entry point runs."""
    from graphpope_amd import sage
    seeds = mc.drawn_seeds(cases.MANUAL_SEED, 1) if p > 0 else [0]
    inp = cases.model_inputs(p, seeds)
    model = cases.build_model(p).to(dev).train()
    adjs = [_adj(dev, (rp, cl), n_src) for rp, cl, n_src in inp.blocks]
    torch.manual_seed(cases.MANUAL_SEED)
    logits = model(inp.x.to(dev), adjs)
    loss = sage.cross_entropy(logits, inp.y.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    got = {"logits": logits.detach().cpu(), "loss": loss.detach().cpu(), "y.0": hidden[0].detach().cpu(),
           "running_mean.0": model.bns[0].running_mean.cpu(), "running_var.0": model.bns[0].running_var.cpu()}
    got.update({"grad:" + k: v.grad.cpu() for k, v in model.named_parameters() if v.grad is not None})
    yard = cases.yardstick(inp, device_on=mc.device_patterns(got, 1))
    rep = mc.check(yard, got, "model p=%s" % p, must_hold=False)
    for k, v in rep["tensors"].items():
        print("%-26s err_dev %.2e  err_32 %.2e  ratio %.2f" % (k, v["err_dev"], v["err_32"], v["ratio"]))
    print("loss err %.2e bound %.2e; gated %s; mismatches %s" % (rep["loss_err"], rep["loss_bound"], rep["gated"], rep["pattern_mismatches"]))
    mc.check(yard, got, "model p=%s" % p)
    assert len(hidden) == 1 and int(model.bns[0].num_batches_tracked) == 1
    assert lib_calls.count("sage_l2_normalize_forward") == lib_calls.count("sage_l2_normalize_backward") == 2
    assert not any(c.endswith("_stats") or c.endswith("_backward_bias") for c in lib_calls), lib_calls
    assert lib_calls.count("sage_bn_relu_dropout_forward") == lib_calls.count("sage_bn_relu_dropout_backward") == 1


# ------------------------------------------------------------------------------------------------ the shortcuts' own shape

def _conv_bn_run(dev, t, blk, normalize):
    from graphpope_amd import sage
    n_dst, n_src, _, c_out = cases.HANDOFF
    conv, adj = _conv(dev, t, normalize), _adj(dev, blk, n_src)
    bn = torch.nn.BatchNorm1d(c_out).to(dev)
    with torch.no_grad():
        bn.weight.copy_(t["gamma"])
        bn.bias.copy_(t["beta"])
    x = t["x"].to(dev).requires_grad_(True)
    y = sage.conv_bn_relu_dropout(conv, bn, (x, x[:n_dst]), adj, 0.0, True)
    (y * t["g"].to(dev)).sum().backward()
    got = dict(_conv_grads(conv, x), out=y.detach().cpu())
    got["grad:gamma"], got["grad:beta"] = bn.weight.grad.cpu(), bn.bias.grad.cpu()
    return got


def test_normalising_conv_takes_neither_shortcut_where_the_plain_one_takes_both(dev, lib_calls):
    """2 000 destinations, 64 -> 128: the plain conv's projection leaves BatchNorm its statistics and BatchNorm's backward pass leaves the
    conv its bias gradient (asserted on the calls).  With normalize=True the statistics pass runs over the normalised rows and the bias
    gradient comes out of sage_conv_backward; output and all six gradients meet the float64 reference, which the restated shortcuts
    miss by more than ten thresholds (test_sage_normalize_cpu.py)."""
    t, blk = cases.conv_bn_inputs()
    _conv_bn_run(dev, t, blk, False)
    assert lib_calls == ["sage_conv_forward_stats", "sage_bn_relu_dropout_forward_stats", "sage_bn_relu_dropout_backward_bias", "sage_conv_backward"]
    del lib_calls[:]
    got = _conv_bn_run(dev, t, blk, True)
    assert lib_calls == ["sage_conv_forward", "sage_l2_normalize_forward", "sage_bn_relu_dropout_forward", "sage_bn_relu_dropout_backward",
                         "sage_l2_normalize_backward", "sage_conv_backward"]
    ref, limit, gated, mismatches = cases.conv_bn_yardstick(t, blk, device_on=got["out"] > 0)
    print("gated", gated, "of", got["out"].numel(), "pattern mismatches outside the gate", mismatches)
    assert gated <= 1e-3 * got["out"].numel() and mismatches == 0
    cases.conv_check(got, ref, limit, "conv+bn normalize")


# ------------------------------------------------------------------------------------------------ inference

@pytest.mark.parametrize("num_layers, hops", [(2, 2), (3, 2), (3, 3)])
def test_inference_equals_eval_mode_forward(dev, lib_calls, num_layers, hops):
    """A 200-node graph (row 2 without a neighbour): SAGE.inference and model.eval()(x, [whole graph] * hops) both within the threshold of
    the float64 eval-mode model, hence of each other within two; inference is the layer call without its BatchNorm epilogue, the
    normalise launch, then the evaluation-mode BatchNorm + ReLU."""
    model = cases.eval_model(num_layers).to(dev).train()
    ref, limit = cases.eval_yardstick(cases.eval_model(num_layers).state_dict(), hops)
    adj = _adj(dev, cases.eval_graph(), cases.EVAL_N)
    x = cases.eval_x().to(dev)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    got = model.inference(x, adj, hops=hops)
    assert lib_calls == (["sage_full_layer_forward", "sage_l2_normalize_forward", "sage_bn_relu_dropout_forward"] * hops)[:-1]
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items()) and model.training and not got.requires_grad
    with torch.no_grad():
        fwd = model.eval()(x, [adj] * hops)
    e_inf, e_fwd, e_both = cases.err(got.cpu(), ref), cases.err(fwd.cpu(), ref), cases.err(got.cpu(), fwd.cpu())
    print("inference %d/%d: err %.3e, eval forward err %.3e, between them %.3e, limit %.3e" % (num_layers, hops, e_inf, e_fwd, e_both, limit))
    assert got.shape == ref.shape == fwd.shape
    assert e_inf <= limit and e_fwd <= limit and e_both <= 2 * limit
    assert torch.equal(model.inference(x, adj, hops=hops), got)


# ------------------------------------------------------------------------------------------------ the replayed steps

@pytest.fixture(scope="module")
def small_graph(dev):
    from graphpope_amd import engine, synth
    ei = synth.powerlaw_graph(300, 1500, seed=5, alpha=0.7, shift=2.0)
    return engine.build_csr(torch.as_tensor(ei, device=dev), 300)


def _train(small_graph, dev, use_graph, state, steps=5):
    from graphpope_amd.optim import Adam
    from graphpope_amd.sage import SAGE
    from graphpope_amd.sampler import NeighborSampler
    from graphpope_amd.train import SageEvalStep, SageTrainStep
    feats = torch.randn(300, 12, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    labels = torch.randint(0, 5, (300,), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    perm = torch.randperm(300, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    sampler = NeighborSampler(small_graph.rowptr, small_graph.col, 300, (3, 2))
    m = SAGE(12, 5, 16, 2, normalize=True).to(dev)
    m.load_state_dict(state)
    opt = Adam(m.parameters(), lr=0.01, max_grad_norm=0.5)
    st = SageTrainStep(m, opt, feats, 64, (3, 2), sampler=sampler, clip=None, graph=use_graph, seed=11)
    losses = []
    for i in range(steps):                                             # with graph=True: two eager warm-up steps, then three replays
        sd = perm[(i % 4) * 64:(i % 4 + 1) * 64].contiguous()
        losses.append(st.step(sd, labels[sd].contiguous()).item())
    assert (st._graph is not None) == use_graph
    ev = SageEvalStep(m, feats, 64, sampler, graph=use_graph)
    passes = [ev.run_pass(perm[:256].contiguous(), labels, 9) for _ in range(2)]           # 4 full batches: the second pass replays throughout
    assert (ev._graph is not None) == use_graph
    torch.cuda.synchronize()
    return losses, {k: v.detach().clone() for k, v in m.state_dict().items()}, passes


def test_replayed_steps_give_the_bits_of_eager_steps(small_graph, dev):
    """SageTrainStep and SageEvalStep, unchanged, on a normalising model in deterministic mode: 300 nodes, batch 64, sizes (3, 2).  Three
    replayed training steps behind the two eager warm-up steps end in the bits of five eager steps -- every loss, parameter and running
    statistic; the evaluation passes give the same loss and accuracy.  The captured launches run over capacity-sized buffers, so this
    holds only because the normalisation reads the true row count on the device."""
    from graphpope_amd import sage
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in sage.SAGE(12, 5, 16, 2, normalize=True).to(dev).state_dict().items()}
    with sage.deterministic():
        eager = _train(small_graph, dev, False, state)
        replayed = _train(small_graph, dev, True, state)
    assert all(np.isfinite(eager[0])) and eager[0] == replayed[0], (eager[0], replayed[0])
    assert eager[1].keys() == replayed[1].keys() and any("running_var" in k for k in eager[1])
    for k in eager[1]:
        assert torch.equal(eager[1][k], replayed[1][k]), k
    assert any(not torch.equal(eager[1][k], state[k]) for k in state if "weight" in k)              # the steps did move the weights
    assert eager[2] == replayed[2] and eager[2][0] == eager[2][1], (eager[2], replayed[2])


# ------------------------------------------------------------------------------------------------ the default is what it was

def test_normalize_false_is_the_two_argument_constructor_bit_for_bit(dev, lib_calls):
    """SAGE(..., normalize=False) and SAGEConv(c_in, c_out, False, True, True) against the constructors without the new arguments: the same
    parameters from the same generator state, the same library calls, and equal bits in the output and in every gradient."""
    from graphpope_amd import sage
    inp = cases.model_inputs(0.5, [0])
    adjs = [_adj(dev, (rp, cl), n_src) for rp, cl, n_src in inp.blocks]
    runs = []
    for kwargs in ({}, {"normalize": False}):
        torch.manual_seed(5)
        model = sage.SAGE(12, 5, 16, 2, dropout=0.5, **kwargs).to(dev).train()
        del lib_calls[:]
        torch.manual_seed(cases.MANUAL_SEED)
        with sage.deterministic():                                     # the inner block's input gradient: no float atomics
            logits = model(inp.x.to(dev), adjs)
            sage.cross_entropy(logits, inp.y.to(dev)).backward()
        runs.append((list(lib_calls), logits.detach(), [p.grad.clone() for p in model.parameters()], [p.detach().clone() for p in model.parameters()]))
    (calls_a, out_a, grads_a, params_a), (calls_b, out_b, grads_b, params_b) = runs
    assert calls_a == calls_b and not any("l2_normalize" in c for c in calls_a)
    assert all(torch.equal(a, b) for a, b in zip(params_a, params_b)) and len(grads_a) == len(grads_b) == 8
    assert torch.equal(out_a.view(torch.int32), out_b.view(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(grads_a, grads_b))
    t, blk = cases.conv_inputs(5, True)
    x, adj = t["x"].to(dev), _adj(dev, blk, cases.N_SRC)
    outs = []
    for args in ((), (False, True, True)):
        torch.manual_seed(9)
        conv = sage.SAGEConv(cases.C_IN, 5, *args).to(dev)
        outs.append(conv((x, x[:cases.N_DST]), adj).detach())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert not torch.allclose(outs[0].norm(dim=1), torch.ones(cases.N_DST, device=dev), atol=1e-3)          # and it is not normalised
