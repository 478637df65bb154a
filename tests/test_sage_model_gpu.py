"""The composed GraphSAGE model on the GPU against the float64 model of tests/sage_model_cases.py (main.py:204-216, 244, 286): logits,
every hidden layer's output, the loss, every parameter gradient and the running statistics of graphpope_amd.sage.SAGE within FACTOR times
the float32 restatement's own error, the ReLU pattern exact outside the gate; then SageTrainStep's clip and Adam on top of it, eagerly and
as a replayed graph.  Every case first pins the kernel paths it was chosen for (sage_forward_kernel_name / sage_backward_kernel_name on
this device, and the record of the library calls).

The batch is read back from the device and is the reference's input; it is also the batch the CPU restatement of the sampler draws, the
one test_sage_model_cpu.py asserts the gate's share on.  The hidden outputs are taken by wrapping sage._bn_forward; under graph replay that
record cannot be trusted (the captured buffers are reused inside the graph), so the training-step test runs the forward layers again under
no_grad on a copy of the pre-step model -- same batch, parameters and seed word -- after asserting that its logits are the step's bit
for bit.  With SAGE_MODEL_PARITY_JSON=<file> the measured figures are written there (profiles/sage_model_parity.json)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import sage_model_cases as mc

pytestmark = pytest.mark.gpu

SEED_WORD = 0x1234_0000_0BAD
MANUAL_SEED = 77


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


@pytest.fixture(scope="module")
def parity_report():
    rep = {}
    yield rep
    path = os.environ.get("SAGE_MODEL_PARITY_JSON")
    if path and rep:
        with open(path, "w") as f:
            json.dump({"factor": mc.FACTOR, "gate": mc.GATE, "edge_permutations": mc.PERMS, "device": torch.cuda.get_device_name(0),
                       "ratio": "err_dev / (factor * err_32): at most 1", "cases": rep}, f, indent=1, sort_keys=True)
            f.write("\n")


@pytest.fixture(scope="module")
def world(dev):
    """name -> the case's graph, sampler, features and labels on the device (and the features on the CPU), built once."""
    from graphpope_amd import engine, synth
    from graphpope_amd.sampler import NeighborSampler
    cache = {}

    def get(name):
        case = mc.CASES[name]
        if case.graph not in cache:
            n, pairs, seed, alpha, shift = case.graph
            ei = synth.powerlaw_graph(n, pairs, seed=seed, alpha=alpha, shift=shift)
            cache[case.graph] = engine.build_csr(torch.as_tensor(ei, device=dev), n)
        csr = cache[case.graph]
        if name not in cache:
            feats = mc.case_features(case)
            cache[name] = (NeighborSampler(csr.rowptr, csr.col, case.graph[0], case.sizes), feats, feats.to(dev), mc.case_labels(case))
        return (case,) + cache[name]
    return get


@pytest.fixture
def lib_calls(monkeypatch):
    """The names of the library calls that enqueue work, in order (as in test_epilogue_gpu.py); `.lib` is the library itself."""
    from graphpope_amd import _lib
    lib = _lib.load()

    class Calls(list):
        pass
    calls = Calls()
    calls.lib = lib

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith("sage_") or name.endswith("_bytes") or name.endswith("_name"):
                return fn
            return lambda *a: (calls.append(name), fn(*a))[1]
    monkeypatch.setattr(_lib, "load", Recorder)
    return calls


@pytest.fixture
def hidden(monkeypatch):
    """[(y, seed, seed word or None, statistics handed over)] of every sage._bn_forward call, in order."""
    from graphpope_amd import sage
    real, seen = sage._bn_forward, []

    def wrapped(lib, x, gamma, beta, t, stats=None):
        out = real(lib, x, gamma, beta, t, stats)
        seen.append((out[0], t.seed, t.seed_dev, stats is not None))
        return out
    monkeypatch.setattr(sage, "_bn_forward", wrapped)
    return seen


def _read_batch(n_id, adjs):
    """(n_id, blocks) at the true sizes from device tensors: host-sized SampledAdjs or the capacity buffers of a DeviceBatch."""
    blocks = []
    for adj in adjs:
        if adj.dims is None:
            n_dst, n_src, nnz = adj.n_dst, adj.n_src, adj.col.numel()
        else:
            n_dst, n_src, nnz = (int(v) for v in adj.dims[:3].cpu())
            assert n_dst <= adj.n_dst and n_src <= adj.n_src and nnz <= adj.col.numel()
        blocks.append((adj.rowptr[:n_dst + 1].cpu().numpy().astype(np.int64), adj.col[:nnz].cpu().numpy().astype(np.int64), n_src))
    return n_id[:blocks[0][2]].cpu().numpy(), blocks


def _same_batch(a, b):
    return np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(
        np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1]) and u[2] == v[2] for u, v in zip(a[1], b[1]))


def _collect(model, logits, loss, ys, blocks):
    got = {"logits": logits.detach().cpu(), "loss": loss.detach().cpu()}
    for i, y in enumerate(ys):
        got["y.%d" % i] = y.detach()[:len(blocks[i][0]) - 1].cpu()
        got["running_mean.%d" % i] = model.bns[i].running_mean.detach().cpu()
        got["running_var.%d" % i] = model.bns[i].running_var.detach().cpu()
    for k, p in model.named_parameters():
        if p.grad is not None:
            got["grad:" + k] = p.grad.detach().cpu()
    return got


def _print_report(name, rep):
    for k, v in rep["tensors"].items():
        print("%-24s %-30s err_dev %.2e  err_32 %.2e  ratio %.2f" % (name, k, v["err_dev"], v["err_32"], v["ratio"]))
    print("%-24s loss err %.2e bound %.2e; gated %s of %s; pattern mismatches %s" % (name, rep["loss_err"], rep["loss_bound"], rep["gated"],
                                                                                   rep["elements"], rep["pattern_mismatches"]))


def _judge(name, inp, got, parity_report):
    yard = mc.yardstick(inp, device_on=mc.device_patterns(got, inp.hidden_layers))
    rep = mc.check(yard, got, name, must_hold=False)
    parity_report[name] = rep
    _print_report(name, rep)
    mc.check(yard, got, name)
    return yard


WAYS = [("M1", "host"), ("M1", "extent"), ("M1", "plain"), ("M2", "host"), ("M2", "extent"), ("M2", "deterministic"), ("M3", "host"),
        ("M3", "extent")]


@pytest.mark.parametrize("name,way", WAYS, ids=["%s-%s" % w for w in WAYS])
def test_model_matches_the_float64_model(name, way, dev, world, lib_calls, hidden, parity_report):
    """host: sampler.sample + IndexedFeatures, the dropout seeds drawn from torch's generator.  extent: sample_device (capacities, true sizes
    in `dims`), the seeds following a device word.  plain: x[n_id] materialised instead of IndexedFeatures.  deterministic: extent under
    sage.set_deterministic(True)."""
    from graphpope_amd import sage
    case, sampler, feats_cpu, feats, labels = world(name)
    extent = way in ("extent", "deterministic")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert mc.planned_names(lib_calls.lib, case, extent, cus) == mc.expected_names(case, extent), "a retune moved this case off its path"
    seeds = torch.as_tensor(mc.case_seeds(case), device=dev)
    y = labels.to(dev)
    model = mc.case_model(case).to(dev).train()
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    n_hidden = len(case.sizes) - 1
    was = sage.set_deterministic(way == "deterministic")
    try:
        if extent:
            b = sampler.sample_device(seeds, seed=case.sample_seed)
            n_id, adjs = b.n_id, b.adjs
            model.dropout_seed_dev = torch.tensor([SEED_WORD], dtype=torch.int64, device=dev)
            want_seeds, word = [mc.layer_seed(i) for i in range(n_hidden)], SEED_WORD
        else:
            n_id, adjs = sampler.sample(seeds, seed=case.sample_seed)
            want_seeds, word = mc.drawn_seeds(MANUAL_SEED, n_hidden), 0
        batch = _read_batch(n_id, adjs)
        assert _same_batch(batch, mc.host_batch(case)), "the device batch is not the one the CPU restatement of the sampler draws"
        x = feats.index_select(0, n_id[:batch[1][0][2]]) if way == "plain" else sage.IndexedFeatures(feats, n_id)
        del lib_calls[:]
        torch.manual_seed(MANUAL_SEED)
        logits = model(x, adjs)
        loss = sage.cross_entropy(logits, y)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        sage.set_deterministic(was)
    # which entry points ran
    handoff = [f.split("<")[0] in ("k_gemm_tile16", "k_gather_beside_gemm") for f, _ in mc.expected_names(case, extent)[:n_hidden]]
    if not extent:
        assert tuple(handoff) == case.bn_calls
    first = "sage_conv_forward_stats" if way == "plain" else "sage_conv_forward_indexed_stats"
    assert lib_calls[0] == first and lib_calls.count("sage_conv_backward") == len(case.sizes)
    assert lib_calls.count("sage_bn_relu_dropout_forward_stats") == lib_calls.count("sage_bn_relu_dropout_backward_bias") == sum(handoff)
    assert lib_calls.count("sage_bn_relu_dropout_forward") == lib_calls.count("sage_bn_relu_dropout_backward") == n_hidden - sum(handoff)
    assert [h[3] for h in hidden] == handoff
    assert [h[1] for h in hidden] == want_seeds and all((h[2] is not None) == extent for h in hidden)
    assert all(int(model.bns[i].num_batches_tracked) == 1 for i in range(n_hidden))
    assert all(p.grad is None for k, p in model.named_parameters() if k.startswith(("convs.%d." % len(case.sizes), "bns.%d." % n_hidden)))
    got = _collect(model, logits, loss, [h[0] for h in hidden], batch[1])
    inp = mc.Inputs(state, feats_cpu[torch.from_numpy(batch[0])], batch[1], labels, want_seeds, word)
    _judge("%s-%s" % (name, way), inp, got, parity_report)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "replayed"])
def test_training_step_matches_float64_model_clip_and_adam(use_graph, dev, world, hidden, parity_report):
    """SageTrainStep on M2's shapes, four steps, steps 1 and 4 checked (with graph=True step 4 is a replay): (1) logits, loss, gradients and
    running statistics against the float64 model on the pre-step parameters, masks from the pre-step dropout word; (2) grad_norm within 2^-23
    of the float64 norm of the device's own gradients, clip_coef the float32 expression bit for bit; (3) every parameter after the step
    against float64 Adam with the pre-step step word, on (pre-step parameter, the device's gradient times coef, pre-step moments), element-wise
    within sage_model_cases.adam_reference's bound."""
    from graphpope_amd import sage
    from graphpope_amd.optim import Adam
    from graphpope_amd.train import SageTrainStep
    case, sampler, feats_cpu, feats, _ = world("M2")
    model = mc.case_model(case).to(dev)
    opt = Adam(model.parameters(), lr=0.01, max_grad_norm=0.5)
    st = SageTrainStep(model, opt, feats, case.batch, case.sizes, sampler=sampler, clip=None, graph=use_graph, seed=11)
    labels = torch.randint(0, mc.CLASSES, (case.graph[0],), generator=torch.Generator().manual_seed(2)).to(dev)
    order = torch.randperm(case.graph[0], generator=torch.Generator().manual_seed(3)).to(dev)
    named = list(model.named_parameters())
    n_hidden = len(case.sizes) - 1
    for k in range(1, 5):
        sd = order[(k - 1) * case.batch:k * case.batch].contiguous()
        if k in (1, 4):
            torch.cuda.synchronize()
            pre = copy.deepcopy(model)
            state = {key: v.detach().cpu().clone() for key, v in model.state_dict().items()}
            moments = [(opt.state[p]["exp_avg"].cpu().numpy().copy(), opt.state[p]["exp_avg_sq"].cpu().numpy().copy()) if "exp_avg" in opt.state[p]
                       else (np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32)) for _, p in named]
            words = st.state.words.cpu().clone()
        st.step(sd, labels[sd].contiguous())
        if k not in (1, 4):
            continue
        torch.cuda.synchronize()
        tag = "step-%s-%d" % ("replayed" if use_graph else "eager", k)
        assert int(words[2]) == k and int(st.state.adam_step) == k + 1
        if use_graph:
            assert (st._graph is not None) == (k == 4), "step 4 must be a replay of the graph captured at step 3"
        batch = _read_batch(st.batch.n_id, st.batch.adjs)
        assert torch.equal(st.batch.n_id[:case.batch], sd)
        # the hidden outputs: the forward layers once more on the pre-step copy
        pre.train()
        pre.dropout_seed_dev = words[0:1].to(dev)
        del hidden[:]
        with torch.no_grad():
            again = pre(sage.IndexedFeatures(feats, st.batch.n_id), st.batch.adjs)
        assert torch.equal(again, st.logits), "the forward pass run again does not give the step's logits bit for bit"
        assert [h[1] for h in hidden] == [mc.layer_seed(i) for i in range(n_hidden)]
        for i in range(n_hidden):
            assert torch.equal(pre.bns[i].running_mean, model.bns[i].running_mean) and torch.equal(pre.bns[i].running_var, model.bns[i].running_var)
            assert int(model.bns[i].num_batches_tracked) == int(state["bns.%d.num_batches_tracked" % i]) + 1
        got = _collect(model, st.logits, st.loss, [h[0] for h in hidden], batch[1])
        inp = mc.Inputs(state, feats_cpu[torch.from_numpy(batch[0])], batch[1], st.y.cpu(), [mc.layer_seed(i) for i in range(n_hidden)],
                        int(words[0]) % (1 << 64))
        _judge(tag, inp, got, parity_report)                          # (1); the gate's share is asserted there, on the float64 model
        # (2)
        grads = [p.grad for _, p in named if p.grad is not None]
        norm64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
        norm = np.float32(opt.grad_norm.item())
        coef = np.float32(opt.clip_coef.item())
        print(tag, "grad_norm %r float64 %r coef %r" % (norm, norm64, coef))
        assert abs(float(norm) - norm64) <= 2.0 ** -23 * norm64
        assert coef.view(np.uint32) == mc.expected_coef(norm, 0.5).view(np.uint32)
        # (3)
        worst = 0.0
        for (key, p), (m0, v0) in zip(named, moments):
            after = p.detach().cpu().numpy()
            if p.grad is None:
                assert np.array_equal(after, state[key].numpy()), key
                continue
            want, bound = mc.adam_reference(state[key].numpy(), p.grad.cpu().numpy(), m0, v0, coef, 0.01, 0.9, 0.999, 1e-8, k)
            ratio = np.abs(after.astype(np.float64) - want) / bound
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (tag, key, float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))
        print(tag, "Adam: worst error / bound %.3f" % worst)
        parity_report[tag]["adam_worst_error_over_bound"] = worst
        parity_report[tag]["grad_norm"] = [float(norm), norm64, float(coef)]
