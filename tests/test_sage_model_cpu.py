"""tests/sage_model_cases.py checked without a GPU.

  * the float64 reference agrees to 1e-12 with code that is not the model's: oracle.sage_conv_torch + torch.nn.BatchNorm1d + relu + a mask
    multiply + F.cross_entropy (main.py:204-216), running statistics included;
  * the share of gated elements of every host-known case is below the cap, on the reference alone;
  * every case's kernel paths, as the library's plan functions print them on 256 compute units, are the ones its table names;
  * the Adam bound holds for a float32 restatement of k_adam's formula and does not hold for a bias correction one step behind;
  * the float32 restatement with one thing wrong at a time, through the very check the GPU test uses, exceeds its threshold tenfold.
The yardstick figures measured here (restatement errors, spread over the edge permutations, gate counts) are printed (-s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_epilogue_cases as bn
import sage_model_cases as mc

SEED_WORD = 0x1234_0000_0BAD


def _inputs(name):
    case = mc.CASES[name]
    return mc.host_inputs(case, [mc.layer_seed(i) for i in range(len(case.sizes) - 1)], SEED_WORD)


@pytest.fixture(scope="module")
def yards():
    """name -> (Inputs, Yardstick): computed once, shared, left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            inp = _inputs(name)
            cache[name] = (inp, mc.yardstick(inp))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(mc.CASES))
def test_reference_equals_torch_modules_in_float64(name, oracle):
    inp = _inputs(name)
    ref = mc.run_model(inp, torch.float64)
    st = {k: v.double().requires_grad_("running" not in k) for k, v in inp.state.items() if v.dtype.is_floating_point}
    h = inp.x.double()
    last = len(inp.blocks) - 1
    for i, (rowptr, col, _) in enumerate(inp.blocks):
        h = oracle.sage_conv_torch(h, torch.from_numpy(rowptr), torch.from_numpy(col), st["convs.%d.lin_l.weight" % i],
                                   st["convs.%d.lin_l.bias" % i], st["convs.%d.lin_r.weight" % i])
        if i == last:
            break
        mod = torch.nn.BatchNorm1d(h.shape[1], eps=mc.EPS, momentum=mc.MOMENTUM).double()
        with torch.no_grad():
            mod.weight.copy_(st["bns.%d.weight" % i])
            mod.bias.copy_(st["bns.%d.bias" % i])
        st["bns.%d.weight" % i], st["bns.%d.bias" % i] = mod.weight, mod.bias
        mod.running_mean.copy_(st["bns.%d.running_mean" % i])
        mod.running_var.copy_(st["bns.%d.running_var" % i])
        h = torch.relu(mod(h)) * inp.keeps[i] / (1 - inp.p)
        assert int(mod.num_batches_tracked) == 1
        for key, got in (("running_mean.%d" % i, mod.running_mean), ("running_var.%d" % i, mod.running_var)):
            assert float((got - ref.out[key]).abs().max()) <= 1e-12 * max(1.0, float(got.abs().max())), key
        assert float((h.detach() - ref.out["y.%d" % i]).abs().max()) <= 1e-12 * max(1.0, float(h.detach().abs().max())), i
    loss = F.cross_entropy(h, inp.y)
    loss.backward()
    assert abs(float(loss.detach()) - float(ref.out["loss"])) <= 1e-12 and float((h.detach() - ref.out["logits"]).abs().max()) <= 1e-12 * float(h.detach().abs().max())
    grads = {k: v for k, v in ref.out.items() if k.startswith("grad:")}
    assert len(grads) == 3 * len(inp.blocks) + 2 * last
    for key, want in grads.items():
        got = st[key[5:]].grad
        scale = ref.grad_h_abs.get(key, max(float(want.abs().max()), 1e-300))
        assert float((got - want).abs().max()) <= 1e-12 * max(scale, 1.0), key
    # the bias in front of a training-mode BatchNorm: zero in exact arithmetic, float64 noise against the sum that cancels
    for key, scale in ref.grad_h_abs.items():
        print(name, key, "float64 |gradient| / sum |grad_h|: %.1e" % (float(ref.out[key].abs().max()) / scale))
        assert float(ref.out[key].abs().max()) <= 1e-13 * scale


@pytest.mark.parametrize("name", list(mc.CASES))
def test_gate_share_and_yardstick_figures(name, yards):
    inp, yard = yards(name)
    for layer, (g, m) in enumerate(zip(yard.gated, yard.elements)):
        print(name, "layer", layer, "gated", g, "of", m)
        assert g <= bn.EXCLUDED_CAP * m
    flips = [int(((z.float() > 0) != p).sum()) for z, p in zip(mc.run_model(inp, torch.float32).z, yard.ref.patterns)]
    print(name, "ReLU flips of the free float32 restatement", flips)
    z_err = [float((a.double() - b).abs().max()) for a, b in zip(mc.run_model(inp, torch.float32, patterns=yard.ref.patterns).z, yard.ref.z)]
    print(name, "float32 error of z per hidden layer", ["%.1e" % e for e in z_err])
    assert max(z_err) < mc.GATE / 16                                   # the gate is wide against what it has to cover
    per_run = []
    for k in range(mc.PERMS):
        r = mc.run_model(inp, torch.float32, patterns=yard.ref.patterns, perm=k)
        per_run.append(mc._errors(r.out, yard.ref, yard.scale))
    for key in yard.scale:
        e = np.array([r[key] for r in per_run])
        print("%s %-32s err_32 max %.2e  max/median %.2f  max/min %.2f" % (name, key, e.max(), e.max() / np.median(e), e.max() / max(e.min(), 1e-300)))
    assert mc.check(yard, mc.run_model(inp, torch.float32, patterns=yard.ref.patterns, perm=3).out, name)["worst"] <= 1.0


@pytest.mark.parametrize("extent", [False, True], ids=["host", "capacity"])
@pytest.mark.parametrize("name", list(mc.CASES))
def test_kernel_paths_of_every_case(name, extent):
    from graphpope_amd import _lib
    case = mc.CASES[name]
    if not extent:
        assert tuple((len(rp) - 1, n_src) for rp, _, n_src in mc.host_batch(case)[1]) == case.host_dims
    assert mc.planned_names(_lib.load(), case, extent) == mc.expected_names(case, extent)


def test_m3_outer_block_is_the_smallest_shape_with_statistics():
    """Among the 256 -> 256 forward shapes the suite uses, 5 800 destinations is the first whose projection runs as whole tiles (the kernels
    that leave BatchNorm's statistics); the backward of that block is a stream-K weight gradient and the inner block takes k_gemm_dual."""
    import ctypes
    from graphpope_amd import _lib
    import sage_backward_cases as sb
    lib = _lib.load()
    used = sorted({s[0] for s, _, _ in sb.FORWARD if s[1:] == (256, 256)} | {5800, 11000, 4096})     # test_every_forward_path_matches_torch
    whole = []
    for n in used:
        buf = ctypes.create_string_buffer(96)
        _lib.check(lib.sage_forward_kernel_name(n, 256, 256, mc.CUS, buf, 96))
        if buf.value.decode().split("<")[0] in ("k_gemm_tile16", "k_gather_beside_gemm"):
            whole.append(n)
    case = mc.CASES["M3"]
    assert min(whole) == 5800 == case.host_dims[0][0] and 257 <= case.host_dims[1][0] <= 4064
    assert "streamk_tn" in case.backward[0][0] and case.backward[1][0].startswith("k_gemm_dual")


def _adam_inputs(n, step, rng):
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-10, 1, n)).astype(np.float32)
    g[:8] = (0.0, 1e-12, -1e-12, 1e-20, 3.0, -3.0, 1e-9, -1e-9)
    if step == 1:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    m = (rng.standard_normal(n) * 10.0 ** rng.uniform(-10, 0, n)).astype(np.float32)
    v = (m.astype(np.float64) ** 2 * rng.uniform(0.5, 50, n)).astype(np.float32)
    return p, g, m, v


@pytest.mark.parametrize("step", [1, 2, 4, 1000])
@pytest.mark.parametrize("coef", [1.0, 0.37])
def test_adam_bound_holds_for_the_float32_restatement(step, coef):
    rng = np.random.default_rng(step)
    p, g, m, v = _adam_inputs(20000, step, rng)
    coef = np.float32(coef)
    want, bound = mc.adam_reference(p, g, m, v, coef, 0.01, 0.9, 0.999, 1e-8, step)
    got, _, _ = mc.adam_restate32(p, g, m, v, coef, 0.01, 0.9, 0.999, 1e-8, step)
    ratio = np.abs(got.astype(np.float64) - want) / bound
    print("step", step, "coef", coef, "restatement error / bound: max %.3f" % ratio.max(), "bound / |p|: median %.1e" % np.median(bound / np.abs(want)))
    assert ratio.max() <= 1.0
    assert np.median(bound / np.maximum(np.abs(want), 1e-3)) < 4e-7         # about three ulps of the parameter: nothing hides under it
    # a bias correction one step behind (or ahead) is far outside
    other, _, _ = mc.adam_restate32(p, g, m, v, coef, 0.01, 0.9, 0.999, 1e-8, step + 1)
    assert np.median(np.abs(other.astype(np.float64) - want) / bound) >= 10.0
    # a gradient applied without the coefficient
    if coef != 1:
        other, _, _ = mc.adam_restate32(p, g, m, v, 1.0, 0.01, 0.9, 0.999, 1e-8, step)
        assert (np.abs(other.astype(np.float64) - want) / bound).max() >= 10.0


def _mutants(inp):
    last = len(inp.blocks) - 1
    return [
        ("one row's mean divided by deg + 1", dict(kind="deg_plus_one", layer=1, row=17)),
        ("one edge of the last row of the inner block dropped", dict(kind="drop_edge")),
        ("1 / (1 - p) missing in one layer's backward", dict(kind="no_rescale_backward", layer=1)),
        ("the layer-1 mask drawn with layer 0's seed in the backward only", dict(kind="backward_mask_seed", layer=1, seed=inp.seeds[0])),
        ("the hidden layer's lin_l.bias gradient taken from grad_y", dict(kind="bias_from_grad_y", layer=last - 1)),
        ("running variance updated with the biased variance", dict(kind="biased_running_var", layer=0)),
        ("grad_x of the inner layer shifted by one row", dict(kind="shift_grad_x")),
    ]


def test_every_mutant_fails_the_check_tenfold(yards):
    """On M2 (two hidden layers with different seeds, an input gradient that came through another layer).  Each mutant is the float32
    restatement with one thing wrong; it goes the way a device result goes: its hidden y give the pattern the gate is resolved with, the
    yardstick is built from the reference side, and check() compares."""
    inp, plain = yards("M2")
    assert int(np.diff(inp.blocks[-1][0])[-1]) > 0
    for label, mutant in _mutants(inp):
        got = mc.run_model(inp, torch.float32, patterns=plain.ref.patterns, perm=2, mutant=mutant).out
        yard = mc.yardstick(inp, device_on=mc.device_patterns(got, inp.hidden_layers))
        assert not any(yard.mismatches), label
        rep = mc.check(yard, got, label, must_hold=False)
        worst = max(rep["tensors"].items(), key=lambda kv: kv[1]["ratio"])
        print("%-70s worst %-30s %.1f x its threshold" % (label, worst[0], worst[1]["ratio"]))
        assert worst[1]["ratio"] >= 10.0, (label, worst)
        with pytest.raises(AssertionError):
            mc.check(yard, got, label)
    # one ReLU pattern element outside the gate flipped: the largest positive pre-activation of layer 1 that the mask keeps is switched off
    z = plain.ref.z[1]
    r, c = np.unravel_index(int(torch.where(inp.keeps[1], z, torch.zeros_like(z)).argmax()), z.shape)
    pats = [p.clone() for p in plain.ref.patterns]
    pats[1][r, c] = False
    got = mc.run_model(inp, torch.float32, patterns=pats, perm=2).out
    yard = mc.yardstick(inp, device_on=mc.device_patterns(got, inp.hidden_layers))
    assert yard.mismatches == [0, 1]
    rep = mc.check(yard, got, "flip", must_hold=False)
    assert rep["tensors"]["y.1"]["ratio"] >= 10.0
    with pytest.raises(AssertionError, match="ReLU pattern"):
        mc.check(yard, got, "flip")


def test_a_flip_inside_the_gate_is_followed_not_failed(yards):
    """An element the gate covers may fall on either side: the reference then differentiates the function the device computed, and the
    comparison stays within the thresholds."""
    inp, plain = yards("M2")
    z = plain.ref.z[0]
    cand = torch.nonzero((z > 0) & (z < mc.GATE) & inp.keeps[0])          # a small positive one, switched off as a float32 z <= 0 would
    assert len(cand) > 0
    r, c = (int(v) for v in cand[0])
    pats = [p.clone() for p in plain.ref.patterns]
    pats[0][r, c] = False
    got = mc.run_model(inp, torch.float32, patterns=pats, perm=1).out
    assert float(got["y.0"][r, c]) == 0.0
    yard = mc.yardstick(inp, device_on=mc.device_patterns(got, inp.hidden_layers))
    assert yard.mismatches == [0, 0] and bool(yard.ref.patterns[0][r, c]) == bool(pats[0][r, c])
    mc.check(yard, got, "flip inside the gate")
