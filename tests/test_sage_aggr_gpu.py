"""SAGEConv(aggr='add' | 'max') and the models built from it on the GPU, through tests/aggr_cases.py: one conv (direct and behind
IndexedFeatures, with and without bias) against the float64 conv; conv + BatchNorm at a shape whose projection hands its statistics over;
one conv per projection path the plan queries show; the two-layer model's loss and every gradient against the float64 model, with the max
gate; SAGE.inference against eval-mode forward; replayed training and evaluation steps against eager ones in both modes of the library;
and aggr='mean' against the constructor without the argument, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import aggr_cases as cases
import sage_model_cases as mc
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


def _conv(dev, t, aggr):
    from graphpope_amd import sage
    conv = sage.SAGEConv(t["w_l"].shape[1], t["w_l"].shape[0], bias="b_l" in t, aggr=aggr).to(dev)
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
@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_conv_against_the_float64_conv(dev, lib_calls, aggr, c_out, bias, way):
    """70 sources, 33 destinations (row 4 without a neighbour), 12 -> c_out: the output and the gradients of x, W_l, b and W_r -- behind
    IndexedFeatures the feature matrix takes none."""
    from graphpope_amd import sage
    t, blk = cases.conv_inputs(c_out, bias)
    ref, limit = cases.conv_yardstick(t, blk, aggr)
    conv, adj = _conv(dev, t, aggr), _adj(dev, blk, cases.N_SRC)
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
    cases.conv_check(got, ref, limit, "conv %s %d %s %s" % (aggr, c_out, "bias" if bias else "nobias", way))
    assert lib_calls == ["sage_conv_forward_indexed_aggr" if way == "indexed" else "sage_conv_forward_aggr", "sage_conv_backward_aggr"]


# ------------------------------------------------------------------------------------------------ conv + BatchNorm: the hand-off stays

@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_conv_and_batchnorm_at_the_hand_off_shape(dev, lib_calls, aggr):
    """2 000 destinations, 64 -> 128: the projection's epilogue leaves BatchNorm its statistics and BatchNorm's backward pass leaves the conv
    its bias gradient, as under the mean -- the hand-off is a property of the projection.  Output and all six gradients against the
    float64 node."""
    from graphpope_amd import sage
    t, blk = cases.sn.conv_bn_inputs()
    n_dst, n_src, _, c_out = cases.HANDOFF
    conv, adj = _conv(dev, t, aggr), _adj(dev, blk, n_src)
    bn = torch.nn.BatchNorm1d(c_out).to(dev)
    with torch.no_grad():
        bn.weight.copy_(t["gamma"])
        bn.bias.copy_(t["beta"])
    x = t["x"].to(dev).requires_grad_(True)
    y = sage.conv_bn_relu_dropout(conv, bn, (x, x[:n_dst]), adj, 0.0, True)
    (y * t["g"].to(dev)).sum().backward()
    got = dict(_conv_grads(conv, x), out=y.detach().cpu())
    got["grad:gamma"], got["grad:beta"] = bn.weight.grad.cpu(), bn.bias.grad.cpu()
    assert lib_calls == ["sage_conv_forward_aggr", "sage_bn_relu_dropout_forward_stats", "sage_bn_relu_dropout_backward_bias", "sage_conv_backward_aggr"]
    ref, limit, gated, mismatches, b_scale = cases.conv_bn_yardstick(t, blk, aggr, device_on=got["out"] > 0)
    print("gated", gated, "of", got["out"].numel(), "pattern mismatches outside the gate", mismatches)
    assert gated <= 1e-3 * got["out"].numel() and mismatches == 0
    cases.conv_bn_check(got, ref, limit, b_scale, "conv+bn %s" % aggr)


# ------------------------------------------------------------------------------------------------ every projection path

# (n_dst, n_src, c_in, c_out) -> what sage_forward_kernel_name / sage_backward_kernel_name (deterministic mode: the form of the grad_x chain
# sage_conv_backward_aggr takes; input and bias gradient wanted) must show on 256 compute units.  The smallest shapes found for each path
# on a grid of widths 16 .. 256 and row counts in steps of 64.  The plain tile kernel with the twin backward is the conv test above, the
# whole-tile kernel with a split-K twin the hand-off test.  NOT reached: the overlapped forward form (k_gather_beside_gemm) -- its gather role
# is the mean's, and the plan never chooses it for another aggregator: at a shape where the mean takes it the projection is one of the forms
# below.
PATHS = {
    "dual": ((320, 480, 16, 16), "k_gemm<64, 64>", "k_gemm_dual<64, 64, 2, 2>[splits=2]+k_bwd_finals"),
    "streamk": ((4096, 4400, 256, 256), "k_gemm_streamk_ld<32>", "k_colsum_partial<true>+k_gemm_streamk_tn<32>[xcd]+k_streamk_tn_fixup<32>"),
}


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_conv_on_every_projection_path(dev, lib, aggr, path):
    from graphpope_amd import _lib, sage
    shape, fwd_name, bwd_name = PATHS[path]
    n_dst, n_src, c_in, c_out = shape
    f, b = ctypes.create_string_buffer(96), ctypes.create_string_buffer(384)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    with sage.deterministic():
        _lib.check(lib.sage_forward_kernel_name(n_dst, c_in, c_out, cus, f, 96))
        _lib.check(lib.sage_backward_kernel_name(n_dst, n_src, c_in, c_out, 1, 1, cus, b, 384))
    print(path, f.value.decode(), "|", b.value.decode())
    assert cus != 256 or (f.value.decode() == fwd_name and b.value.decode().startswith(bwd_name) and "k_scatter_sum_det" in b.value.decode())
    t, blk = cases.conv_inputs(c_out, True, (n_dst, n_src, c_in))
    ref, limit = cases.conv_yardstick(t, blk, aggr)
    conv, adj = _conv(dev, t, aggr), _adj(dev, blk, n_src)
    x = t["x"].to(dev).requires_grad_(True)
    out = conv((x, x[:n_dst]), adj)
    (out * t["g"].to(dev)).sum().backward()
    cases.conv_check(dict(_conv_grads(conv, x), out=out.detach().cpu()), ref, limit, "conv %s %s" % (aggr, path))


# ------------------------------------------------------------------------------------------------ the two-layer model

def _model_run(dev, aggr, inp, hidden, deterministic):
    from graphpope_amd import sage
    model = cases.build_model(aggr).to(dev).train()
    adjs = [_adj(dev, (rp, cl), n_src) for rp, cl, n_src in inp.blocks]
    torch.manual_seed(cases.MANUAL_SEED)
    del hidden[:]
    with sage.deterministic(deterministic):
        logits = model(inp.x.to(dev), adjs)
        loss = sage.cross_entropy(logits, inp.y.to(dev))
        loss.backward()
    torch.cuda.synchronize()
    got = {"logits": logits.detach().cpu(), "loss": loss.detach().cpu(), "y.0": hidden[0].detach().cpu(),
           "running_mean.0": model.bns[0].running_mean.cpu(), "running_var.0": model.bns[0].running_var.cpu()}
    got.update({"grad:" + k: v.grad.cpu() for k, v in model.named_parameters() if v.grad is not None})
    return model, got


@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_two_layer_model_against_the_float64_model(dev, lib_calls, hidden, aggr):
    """SAGE(12, 5, 16, 2, aggr=...) in training mode with dropout 0.5, blocks (40, 90) and (16, 40): logits, loss, the hidden activations,
    the running statistics and every parameter gradient under the rule of sage_model_cases.py.  max: the arg the device used in the inner
    block (restated from its own hidden activations) equals the reference's outside the max gate, and the gate holds no element for these
    seeds.  Both aggregators give the same bits with deterministic mode on and off."""
    inp = cases.model_inputs(cases.model_seeds())
    model, got = _model_run(dev, aggr, inp, hidden, False)
    assert [c for c in lib_calls if "deterministic" not in c] == [          # (the mode's own switch is a recorded call too)
        "sage_conv_forward_aggr", "sage_bn_relu_dropout_forward", "sage_conv_forward_aggr", "sage_cross_entropy_forward",
        "sage_cross_entropy_backward", "sage_conv_backward_aggr", "sage_bn_relu_dropout_backward", "sage_conv_backward_aggr"]
    device_arg = None
    if aggr == "max":
        rowptr, col, _ = inp.blocks[1]
        device_arg = [None, cases.gather_restate(rowptr, col, got["y.0"].numpy(), "max")[1]]
    yard, args, ties = cases.yardstick(inp, aggr, device_on=mc.device_patterns(got, 1), device_arg=device_arg)
    rep = mc.check(yard, got, "model %s" % aggr, must_hold=False)
    for k, v in rep["tensors"].items():
        print("%-26s err_dev %.2e  err_32 %.2e  ratio %.2f" % (k, v["err_dev"], v["err_32"], v["ratio"]))
    print("loss err %.2e bound %.2e; gated %s; mismatches %s" % (rep["loss_err"], rep["loss_bound"], rep["gated"], rep["pattern_mismatches"]))
    if aggr == "max":
        cases.arg_gate_check(args, ties, device_arg, "model max")
    mc.check(yard, got, "model %s" % aggr)
    assert len(hidden) == 1 and int(model.bns[0].num_batches_tracked) == 1
    _, again = _model_run(dev, aggr, inp, hidden, True)
    assert got.keys() == again.keys() and all(torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)) for k in got), aggr


# ------------------------------------------------------------------------------------------------ inference

@pytest.mark.parametrize("num_layers, hops", [(2, 2), (3, 2), (3, 3)])
@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_inference_equals_eval_mode_forward(dev, lib_calls, aggr, num_layers, hops):
    """A 200-node graph (row 2 without a neighbour): SAGE.inference and model.eval()(x, [whole graph] * hops) both within the threshold of
    the float64 eval-mode model; inference is the conv over the whole CSR (aggregate first), then the evaluation-mode BatchNorm + ReLU --
    the launches of forward(), so the two agree to the bit."""
    model = cases.eval_model(num_layers, aggr).to(dev).train()
    ref, limit = cases.eval_yardstick(cases.eval_model(num_layers, aggr).state_dict(), hops, aggr)
    adj = _adj(dev, cases.eval_graph(), cases.EVAL_N)
    x = cases.eval_x().to(dev)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    got = model.inference(x, adj, hops=hops)
    assert lib_calls == (["sage_conv_forward_aggr", "sage_bn_relu_dropout_forward"] * hops)[:-1]
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items()) and model.training and not got.requires_grad
    with torch.no_grad():
        fwd = model.eval()(x, [adj] * hops)
    e_inf, e_fwd = cases.err(got.cpu(), ref), cases.err(fwd.cpu(), ref)
    print("inference %s %d/%d: err %.3e, eval forward err %.3e, limit %.3e" % (aggr, num_layers, hops, e_inf, e_fwd, limit))
    assert got.shape == ref.shape == fwd.shape
    assert e_inf <= limit and e_fwd <= limit
    assert torch.equal(got.view(torch.int32), fwd.view(torch.int32)) and torch.equal(model.inference(x, adj, hops=hops), got)


def test_inference_takes_a_csr_of_the_engine(dev):
    """engine.build_csr pads col behind its last edge: inference over the Csr equals inference over the SampledAdj of the same edges."""
    from graphpope_amd import engine, sage
    rowptr, col = cases.eval_graph()
    dst = np.repeat(np.arange(cases.EVAL_N), np.diff(rowptr))
    order = np.lexsort((col, dst))
    csr = engine.build_csr(torch.from_numpy(np.stack([dst[order], col[order]])).to(dev), cases.EVAL_N)
    adj = sage.SampledAdj(csr.rowptr, csr.col[:int(csr.num_edges)], cases.EVAL_N)
    model = cases.eval_model(2, "max").to(dev)
    x = cases.eval_x().to(dev)
    assert torch.equal(model.inference(x, csr), model.inference(x, adj))


# ------------------------------------------------------------------------------------------------ the replayed steps

@pytest.fixture(scope="module")
def small_graph(dev):
    from graphpope_amd import engine, synth
    ei = synth.powerlaw_graph(300, 1500, seed=5, alpha=0.7, shift=2.0)
    return engine.build_csr(torch.as_tensor(ei, device=dev), 300)


def _train(small_graph, dev, use_graph, state, aggr, steps=5):
    from graphpope_amd.optim import Adam
    from graphpope_amd.sage import SAGE
    from graphpope_amd.sampler import NeighborSampler
    from graphpope_amd.train import SageEvalStep, SageTrainStep
    feats = torch.randn(300, 12, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    labels = torch.randint(0, 5, (300,), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    perm = torch.randperm(300, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    sampler = NeighborSampler(small_graph.rowptr, small_graph.col, 300, (3, 2))
    m = SAGE(12, 5, 16, 2, aggr=aggr).to(dev)
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


@pytest.mark.parametrize("aggr", cases.AGGRS)
def test_replayed_steps_give_the_bits_of_eager_steps_in_both_modes(small_graph, dev, aggr):
    """SageTrainStep and SageEvalStep, unchanged: 300 nodes, batch 64, sizes (3, 2).  Three replayed training steps behind the two eager
    warm-up steps end in the bits of five eager steps -- every loss, parameter and running statistic -- with deterministic mode on AND off:
    the ordered sum has no float atomic in either.  The captured launches run over capacity-sized buffers, so this holds only because
    both kernels read the true extents on the device.  (The evaluation metrics add with one atomic per block outside deterministic mode:
    the passes are compared in it.)"""
    from graphpope_amd import sage
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in sage.SAGE(12, 5, 16, 2, aggr=aggr).to(dev).state_dict().items()}
    runs = {}
    for mode in (True, False):
        with sage.deterministic(mode):
            runs[mode] = (_train(small_graph, dev, False, state, aggr), _train(small_graph, dev, True, state, aggr))
    for mode, (eager, replayed) in runs.items():
        assert all(np.isfinite(eager[0])) and eager[0] == replayed[0], (mode, eager[0], replayed[0])
        assert eager[1].keys() == replayed[1].keys() and any("running_var" in k for k in eager[1])
        for k in eager[1]:
            assert torch.equal(eager[1][k], replayed[1][k]), (mode, k)
        assert any(not torch.equal(eager[1][k], state[k]) for k in state if "weight" in k)          # the steps did move the weights
    eager, replayed = runs[True]
    assert eager[2] == replayed[2] and eager[2][0] == eager[2][1], (eager[2], replayed[2])
    assert runs[True][0][0] == runs[False][0][0]                       # the mode changes nothing for add and max
    assert all(torch.equal(runs[True][0][1][k], runs[False][0][1][k]) for k in state)


# ------------------------------------------------------------------------------------------------ the default is what it was

def test_aggr_mean_is_the_constructor_without_the_argument_bit_for_bit(dev, lib_calls):
    """SAGE(..., aggr='mean') and SAGEConv(c_in, c_out, False, True, True, 'mean') against the constructors without the new argument: the
    same parameters from the same generator state, the same library calls in the same order -- none of the new entry points -- and equal
    bits in the output and in every gradient."""
    from graphpope_amd import sage
    inp = cases.model_inputs([0])
    adjs = [_adj(dev, (rp, cl), n_src) for rp, cl, n_src in inp.blocks]
    runs = []
    for kwargs in ({}, {"aggr": "mean"}):
        torch.manual_seed(5)
        model = sage.SAGE(12, 5, 16, 2, dropout=0.5, **kwargs).to(dev).train()
        del lib_calls[:]
        torch.manual_seed(cases.MANUAL_SEED)
        with sage.deterministic():                                     # the inner block's input gradient: no float atomics
            logits = model(inp.x.to(dev), adjs)
            sage.cross_entropy(logits, inp.y.to(dev)).backward()
        runs.append((list(lib_calls), logits.detach(), [p.grad.clone() for p in model.parameters()], [p.detach().clone() for p in model.parameters()]))
    (calls_a, out_a, grads_a, params_a), (calls_b, out_b, grads_b, params_b) = runs
    assert calls_a == calls_b and not any("aggr" in c for c in calls_a)
    assert sum(c.startswith("sage_conv_forward") for c in calls_a) == 2 and calls_a.count("sage_conv_backward") == 2
    assert all(torch.equal(a, b) for a, b in zip(params_a, params_b)) and len(grads_a) == len(grads_b) == 8
    assert torch.equal(out_a.view(torch.int32), out_b.view(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(grads_a, grads_b))
    t, blk = cases.conv_inputs(5, True)
    x, adj = t["x"].to(dev), _adj(dev, blk, cases.N_SRC)
    outs = []
    for args in ((), (False, True, True, "mean")):
        torch.manual_seed(9)
        conv = sage.SAGEConv(cases.C_IN, 5, *args).to(dev)
        outs.append(conv((x, x[:cases.N_DST]), adj).detach())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    add = sage.SAGEConv(cases.C_IN, 5, aggr="add").to(dev)
    add.load_state_dict(conv.state_dict())
    assert not torch.allclose(add((x, x[:cases.N_DST]), adj), outs[0], atol=1e-3)                  # and another aggregator is another layer
