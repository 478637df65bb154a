"""Every entry point on operands that are 4-byte but not 16-byte aligned (include/graphpope_hip.h, "Alignment"): the scalar kernel,
template instance or plan each call falls back to, through the C ABI with buffers the test owns.

Each run first asserts the path -- the *_kernel_name_at query, the launch code's own plan printed, must print the string of
tests/misaligned_cases.py -- then the values against the same references the aligned tests use (exact where the aligned tests are
exact), then that the guard floats around every placed operand (tests/misaligned.py) still hold their sentinel: a vector access that
rounded its address would show there.  One operand is misaligned at a time, plus one run with all of them; element offset 1 everywhere,
2 (8 bytes) once per family.  These are supported inputs: nothing here is meant to provoke anything."""
import ctypes
import math

import numpy as np
import pytest
import torch

import deterministic_cases as det_cases
import misaligned
import misaligned_cases as cases
import pairwise_cases as pc
import pairwise_plan_cases as pw
import sage_backward_cases as bw
import sage_model_cases as mc
from misaligned import SENTINEL
from test_sage_model_gpu import hidden, parity_report, world  # noqa: F401  (fixtures of the model test)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


@pytest.fixture(scope="module")
def lib():
    from graphpope_amd import _lib
    return _lib.load()


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _name(fn, *args):
    from graphpope_amd import _lib
    buf = ctypes.create_string_buffer(384)
    _lib.check(fn(*args, buf, 384))
    return buf.value.decode()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _assert_guards(placed, tag):
    for name, view in placed.items():
        assert misaligned.guards_intact(view), (tag, name, "the floats around the operand were written")


# ---- SAGE forward ---------------------------------------------------------------------------------------------------------------
def _forward_run(lib, dev, shape, mode, operand, off, true_n=None):
    """sage_conv_forward / _indexed at `shape` with `operand` at element offset `off`; true_n: a capacity-sized call with `dims`."""
    from graphpope_amd import _lib
    p = _lib.ptr
    cap, c_in, c_out = shape
    indexed, extents = mode == "indexed", true_n is not None
    n = true_n if extents else cap
    ref = bw.forward_reference(n, c_in, c_out)
    ref.assert_exact_family_is_exact()
    mask = cases.FORWARD_OPERANDS[mode][operand]
    assert _name(lib.sage_forward_kernel_name_at, cap, c_in, c_out, _cus(dev), mask) == cases.forward_name(shape, mode, operand)
    names = ["x", "agg", "w_l", "w_r", "out", "b_l"] + (["x_dst"] if indexed and operand != "x_dst_null" else [])
    which = set(names) if operand == "all" else {operand} & set(names)
    o = lambda name: off if name in which else 0
    n_src_cap = cap + bw.FORWARD_EXTRA if extents else ref.n_src
    n_rows, nnz_cap = n_src_cap + 500, ref.nnz + (64 if extents else 0)
    rs = np.random.RandomState(n)
    rowptr, col = bw.padded_csr(ref.rowptr, ref.col, cap, nnz_cap, ref.n_src, n_src_cap, rs)
    if indexed:
        feats, n_id = bw.indexed_rows(ref.x, n_rows, n_src_cap, c_in, rs)
        nid_d = torch.from_numpy(n_id).to(dev)
    else:
        feats = bw.nan_padded(ref.x, n_src_cap)
    t = {"x": misaligned.place(feats, dev, o("x")), "w_l": misaligned.place(ref.w_l, dev, o("w_l")), "w_r": misaligned.place(ref.w_r, dev, o("w_r")),
         "b_l": misaligned.place(ref.b, dev, o("b_l")), "agg": misaligned.place(np.full((cap, c_in), SENTINEL), dev, o("agg")),
         "out": misaligned.place(np.full((cap, c_out), SENTINEL), dev, o("out"))}
    if "x_dst" in names:
        t["x_dst"] = misaligned.place(np.full((cap, c_in), SENTINEL), dev, o("x_dst"))
    for name in which:
        assert t[name].data_ptr() % 16 == 4 * off
    rp_d, col_d = torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev)
    dims = torch.tensor([n, ref.n_src, ref.nnz, 0], dtype=torch.int32, device=dev) if extents else None
    sbytes = (lib.sage_conv_forward_indexed_scratch_bytes if indexed else lib.sage_conv_forward_scratch_bytes)(cap, c_in, c_out)
    scratch = torch.empty(max(sbytes, 16), dtype=torch.uint8, device=dev)
    nnz = nnz_cap if extents else ref.nnz
    if indexed:
        _lib.check(lib.sage_conv_forward_indexed(p(rp_d), p(col_d), p(nid_d), n_src_cap, cap, nnz, p(t["x"]), n_rows, c_in, p(t["w_l"]), p(t["b_l"]),
                                                 p(t["w_r"]), c_out, p(t["agg"]), p(t.get("x_dst")), p(t["out"]), p(scratch), sbytes, p(dims), _stream()))
    else:
        _lib.check(lib.sage_conv_forward(p(rp_d), p(col_d), n_src_cap, cap, nnz, p(t["x"]), c_in, p(t["w_l"]), p(t["b_l"]), p(t["w_r"]), c_out,
                                         p(t["agg"]), p(t["out"]), p(scratch), sbytes, p(dims), _stream()))
    torch.cuda.synchronize()
    tag = (shape, mode, operand, off, true_n)
    want = [("agg", ref.agg), ("out", ref.out)] + ([("x_dst", ref.x[:n].astype(np.float64))] if "x_dst" in t else [])
    for what, w in want:
        got = t[what].cpu().numpy().astype(np.float64)
        assert np.array_equal(got[:n], w), (tag, what, int((got[:n] != w).sum()))
        assert np.array_equal(got[n:], np.full_like(got[n:], SENTINEL)), (tag, what, "rows past the true count were written")
    _assert_guards(t, tag)


_FORWARD = [(s, m, o, 1) for s, m, o in cases.FORWARD_ROWS] + [((4160, 256, 256), "plain", "all", 2), ((5800, 256, 256), "indexed", "all", 2)]


@pytest.mark.parametrize("shape,mode,operand,off", _FORWARD, ids=["%dx%d-%d-%s-%s-off%d" % (s + (m, o, f)) for s, m, o, f in _FORWARD])
def test_forward_is_exact_with_a_misaligned_operand(shape, mode, operand, off, dev, lib):
    """agg, out (and x_dst) equal ForwardReference bit for bit whichever operand is off a 16-byte boundary: the projection falls from the
    stream-K, overlapped and whole-tile forms to k_gemm<..., 0, 0>, the gather to k_gather_mean<false>; `out` and `b_l`, which no flag
    covers, change nothing on the vector paths."""
    _forward_run(lib, dev, shape, mode, operand, off)


@pytest.mark.parametrize("mode", ["plain", "indexed"])
def test_forward_with_device_extents_and_a_misaligned_source_matrix(mode, dev, lib):
    """The capacity-sized call with `dims`: exact on the true rows, sentinel behind them, no trace of the NaN rows past the true sources."""
    _forward_run(lib, dev, (4160, 256, 256), mode, "x", 1, true_n=bw.forward_trues(4160)[0])


# ---- SAGE backward --------------------------------------------------------------------------------------------------------------
def _backward_run(lib, dev, case, operand, off, mask, want_name):
    import test_sage_backward_gpu as bwd
    (n, c_in, c_out), extra = case["shape"], case["extra"]
    at = lambda m: _name(lib.sage_backward_kernel_name_at, n, n + extra, c_in, c_out, int(case["grad_x"]), int(case["grad_b"]), _cus(dev), m)
    base = cases.B_INDEXED if case["indexed"] else 0
    assert at(mask) == want_name, (case["id"], operand)
    names = [k for k in cases.BACKWARD_OPERANDS if k != "all" and (k != "grad_x" or case["grad_x"])]
    which = names if operand == "all" else [operand]
    ref = bw.reference(case, n)
    buffers = bwd.Buffers(case, dev, ref.nnz, offsets={k: off for k in which})
    for k in which:
        assert buffers.placed[k].data_ptr() % 16 == 4 * off
    buffers.load(ref, extents=False)
    bwd._check(case, ref, buffers.run(lib), "%s at offset %d" % (operand, off))
    _assert_guards(buffers.placed, (case["id"], operand, off))
    return at(base)


_BACKWARD = [(shape, extra, operand, family, 1) for family in ("exact", "rounding") for shape, operand, extra in cases.BACKWARD_ROWS]
_BACKWARD += [((4064, 256, 256), 300, "all", "exact", 2)]


@pytest.mark.parametrize("shape,extra,operand,family,off", _BACKWARD, ids=["%dx%d-%d+%d-%s-%s-off%d" % (s + (e, o, f, off)) for s, e, o, f, off in _BACKWARD])
def test_backward_with_a_misaligned_operand(shape, extra, operand, family, off, dev, lib):
    """Every gradient on the stream-K, dual, twin and 128 x 256 shapes with one operand (or all) misaligned: the exact family bit for bit,
    the rounding family within Reference.bounds (derived for any order of the additions, so they hold on the fallback path as they are).
    The name differs from the aligned one exactly where the table says so."""
    case = bw._case(shape, extra, family=family)
    want = cases.backward_name(shape, operand, extra)
    aligned = _backward_run(lib, dev, case, operand, off, cases.BACKWARD_OPERANDS[operand], want)
    assert aligned == bw.expected_name(shape, extra)
    assert (want != aligned) == (operand in ("g", "agg", "x", "w_l", "w_r", "all"))


@pytest.mark.parametrize("extra", [0, 300])
def test_backward_indexed_with_a_misaligned_feature_matrix(extra, dev, lib):
    """sage_conv_backward_indexed at layer 0: stream-K, which would read the rows through n_id 16 bytes at a time, is refused; k_gather_rows
    copies them (scalar) into the scratch and the split-K twin runs on vector layouts."""
    case = bw._case(cases.INDEXED_SHAPE, extra, grad_x=False, indexed=True)
    aligned = _backward_run(lib, dev, case, "x", 1, *cases.INDEXED_X)
    assert aligned == cases.INDEXED_ALIGNED[1] != cases.INDEXED_X[1]


# ---- the deterministic sum ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["grad_agg", "grad_x"])
@pytest.mark.parametrize("c,off", [(256, 1), (4, 1), (256, 2)])
def test_det_sum_equals_its_contract_with_a_misaligned_operand(c, off, which, dev, lib):
    """sage_scatter_mean_det on the hand-built block (lists of 0 .. 129 entries) with grad_agg, then grad_x, off a 16-byte boundary at a
    width that otherwise takes 16-byte accesses: bit for bit the float32 loop of the contract."""
    from graphpope_amd import _lib
    rowptr, col = det_cases.hand_built_block()
    n_dst, n_src = det_cases.N_DST, det_cases.N_SRC
    rs = np.random.RandomState(c)
    gagg = rs.randn(n_dst, c).astype(np.float32)
    gx = np.full((n_src, c), SENTINEL, dtype=np.float32)
    gx[:n_dst] = rs.randn(n_dst, c)
    want = det_cases.scatter_mean_reference(rowptr, col, n_src, n_dst, gagg, gx)
    t = {"grad_agg": misaligned.place(gagg, dev, off if which == "grad_agg" else 0), "grad_x": misaligned.place(gx, dev, off if which == "grad_x" else 0)}
    assert t[which].data_ptr() % 16 == 4 * off
    rp_d, col_d = torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev)
    need = lib.sage_scatter_mean_det_scratch_bytes(n_src, n_dst, len(col))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    _lib.check(lib.sage_scatter_mean_det(_lib.ptr(rp_d), _lib.ptr(col_d), n_src, n_dst, len(col), _lib.ptr(t["grad_agg"]), c, _lib.ptr(t["grad_x"]),
                                         _lib.ptr(scratch), need, None, _stream()))
    torch.cuda.synchronize()
    got = t["grad_x"].cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), int((got.view(np.int32) != want.view(np.int32)).sum())
    _assert_guards(t, (c, off, which))


@pytest.mark.parametrize("family", ["exact", "rounding"])
@pytest.mark.parametrize("extra", [0, 300])
def test_backward_in_deterministic_mode_with_a_misaligned_grad_x(extra, family, dev, lib):
    """The stream-K shape with the switch on and grad_x misaligned: the chain ends in k_scatter_sum_det<false>, the gradients are what they
    are on the aligned path."""
    assert lib.sage_get_deterministic() == 0, "an earlier test left the switch on"
    lib.sage_set_deterministic(1)
    try:
        case = bw._case(cases.DET_SHAPE, extra, family=family)
        mask, want = cases.DET_ROWS[1]
        assert mask == cases.B_GX and want.endswith("k_scatter_sum_det<false>")
        aligned = _backward_run(lib, dev, case, "grad_x", 1, mask, want)
        assert aligned == cases.DET_ROWS[0][1]
    finally:
        lib.sage_set_deterministic(0)


# ---- the optimiser --------------------------------------------------------------------------------------------------------------
class _Flat:
    """Tensors of the given (length, element offset) pairs as views into one SENTINEL-filled buffer, eight or more sentinel floats between
    two of them; untouched(): everything outside the views still holds the sentinel."""

    def __init__(self, table, dev, fill):
        pos, self.spans = 0, []
        for n, off in table:
            pos = (pos + misaligned.GUARD + 3) // 4 * 4 + off
            self.spans.append((pos, n))
            pos += n
        self.flat = torch.full((pos + misaligned.GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        assert self.flat.data_ptr() % 16 == 0
        self.views = [self.flat[a:a + n] for a, n in self.spans]
        for (n, off), v, values in zip(table, self.views, fill):
            assert v.data_ptr() % 16 == 4 * off and len(values) == n
            v.copy_(torch.from_numpy(values))

    def pointers(self):
        return (ctypes.c_void_p * len(self.views))(*[v.data_ptr() for v in self.views])

    def untouched(self):
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        for a, n in self.spans:
            keep[a:a + n] = False
        return bool((self.flat[keep] == SENTINEL).all())

    def numpy(self):
        return [v.cpu().numpy() for v in self.views]


_TABLE = [(n, off) for n in cases.ADAM_LENGTHS for off in (0, 1, 2, 3)]
_ALIGNED = [(n, 0) for n, _ in _TABLE]
_NAN_AT = (_TABLE.index((4099, 1)), 4097)                              # tensor, element: in the second chunk of its tensor


def _state(nan):
    rs = np.random.RandomState(11)
    f = lambda scale, n: (rs.randn(n) * scale).astype(np.float32)
    st = dict(p=[f(1.0, n) for n, _ in _TABLE], g=[f(0.1, n) for n, _ in _TABLE], m=[f(0.01, n) for n, _ in _TABLE],
              v=[(rs.rand(n) * 1e-3).astype(np.float32) for n, _ in _TABLE])
    if nan:
        st["g"][_NAN_AT[0]][_NAN_AT[1]] = np.nan
    return st


def _adam_call(lib, dev, st, tables, clip, weight_decay):
    """One step on flat buffers laid out by `tables` ({p, g, m, v}: (length, offset) pairs).  Returns the new (p, m, v) per tensor, the
    float64 partial sums of squares and (norm, coefficient) of a clipping step, after checking the sentinels between the tensors."""
    from graphpope_amd import _lib
    flats = {k: _Flat(tables[k], dev, st[k]) for k in "pgmv"}
    n = len(_TABLE)
    nn = (ctypes.c_int64 * n)(*[length for length, _ in _TABLE])
    hyper = (1e-3, 0.9, 0.999, 1e-8, weight_decay, 3)
    parts, norm_out = None, None
    if clip:
        n_parts = int(lib.sage_grad_norm_partials(n, nn))
        ws = torch.zeros(256, dtype=torch.float64, device=dev)
        norm_out = torch.zeros(2, dtype=torch.float32, device=dev)
        _lib.check(lib.sage_grad_sqnorm(n, flats["g"].pointers(), nn, _lib.ptr(ws), n_parts, _stream()))
        _lib.check(lib.sage_adam_step_clip(n, flats["p"].pointers(), flats["g"].pointers(), flats["m"].pointers(), flats["v"].pointers(), nn, *hyper,
                                           None, 0.5, _lib.ptr(ws), n_parts, _lib.ptr(norm_out), None, 0, None, _stream()))
        torch.cuda.synchronize()
        parts, norm_out = ws[:n_parts].cpu().numpy(), norm_out.cpu().numpy()
    else:
        _lib.check(lib.sage_adam_step(n, flats["p"].pointers(), flats["g"].pointers(), flats["m"].pointers(), flats["v"].pointers(), nn, *hyper, None,
                                      _stream()))
        torch.cuda.synchronize()
    for k, fl in flats.items():
        assert fl.untouched(), (k, "floats between the tensors were written")
    got_g = flats["g"].numpy()
    for a, b in zip(got_g, st["g"]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "the gradients were modified"
    return {k: flats[k].numpy() for k in "pmv"}, parts, norm_out


@pytest.mark.parametrize("nan", [False, True], ids=["numbers", "nan_gradient"])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("clip", [False, True], ids=["step", "step_clip"])
@pytest.mark.parametrize("which", ["p", "g", "mv"])
def test_adam_step_on_views_at_every_offset(which, clip, weight_decay, nan, dev, lib):
    """sage_adam_step / sage_grad_sqnorm + sage_adam_step_clip on 28 tensors (lengths around the chunk of 4096, the pack of four and the
    block, each at element offsets 0 .. 3 of one flat buffer) with p, g or m and v misaligned: p, m, v element by element within the bound
    misaligned_cases.adam_reference derives from update()'s roundings; the squared norm within n 2^-53 of the float64 sum; a NaN gradient
    element poisons what it poisons in the aligned call (its own element; under the clip, through the norm, everything)."""
    st = _state(nan)
    tables = {k: _TABLE if k in which else _ALIGNED for k in "pgmv"}
    got, parts, norm_out = _adam_call(lib, dev, st, tables, clip, weight_decay)
    aligned, _, _ = _adam_call(lib, dev, st, {k: _ALIGNED for k in "pgmv"}, clip, weight_decay)
    coef = None
    if clip:
        squares = [float(x) * float(x) for g in st["g"] for x in g]
        n_elems = len(squares)
        if nan:
            assert np.isnan(parts).any() and np.isnan(norm_out).all()
        else:
            total = math.fsum(squares)
            assert abs(math.fsum(parts) - total) <= n_elems * 2.0 ** -53 * total, (math.fsum(parts), total)
            want_coef, rel = cases.clip_coefficient(math.sqrt(total), 0.5)
            assert want_coef < 1.0 and abs(float(norm_out[1]) - want_coef) <= rel * want_coef, (norm_out, want_coef)
            assert abs(float(norm_out[0]) - math.sqrt(total)) <= 2 * cases.U * math.sqrt(total)
        coef = norm_out[1]
    worst = dict(p=0.0, m=0.0, v=0.0)
    for i in range(len(_TABLE)):
        want, bound = cases.adam_reference(st["p"][i], st["g"][i], st["m"][i], st["v"][i], 1e-3, 0.9, 0.999, 1e-8, weight_decay, 3, coef)
        for k in "pmv":
            g = got[k][i]
            assert np.array_equal(np.isnan(g), np.isnan(want[k])) and np.array_equal(np.isnan(g), np.isnan(aligned[k][i])), (k, _TABLE[i])
            if nan and not clip:
                assert int(np.isnan(g).sum()) == (1 if i == _NAN_AT[0] else 0) and (i != _NAN_AT[0] or np.isnan(g[_NAN_AT[1]]))
            worst[k] = max(worst[k], cases.worst_ratio(g, want[k], bound[k]))
    print("adam err/bound %s clip=%d wd=%g nan=%d: %s" % (which, clip, weight_decay, nan, ", ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst
    if nan and clip:
        assert all(np.isnan(a).all() for k in "pmv" for a in got[k])
    else:
        assert worst["p"] > 0


@pytest.mark.parametrize("which", ["dst", "src", "both"])
def test_copy_segments_on_views_at_every_offset(which, dev, lib):
    """sage_copy_segments between views at element offsets 0 .. 3: the copies are exact and nothing outside them is written."""
    from graphpope_amd import _lib
    rs = np.random.RandomState(5)
    values = [rs.randn(n).astype(np.float32) for n, _ in _TABLE]
    zeros = [np.zeros(n, dtype=np.float32) for n, _ in _TABLE]
    src = _Flat(_TABLE if which in ("src", "both") else _ALIGNED, dev, values)
    dst = _Flat(_TABLE if which in ("dst", "both") else _ALIGNED, dev, zeros)
    n = len(_TABLE)
    nbytes = (ctypes.c_int64 * n)(*[4 * length for length, _ in _TABLE])
    _lib.check(lib.sage_copy_segments(n, dst.pointers(), src.pointers(), nbytes, _stream()))
    torch.cuda.synchronize()
    for a, b in zip(dst.numpy(), values):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert dst.untouched() and src.untouched()


def _repoint(model, dev, every_other):
    """The model's parameters as views into one flat buffer; every_other: odd-numbered parameters one float past a 16-byte boundary."""
    params = list(model.parameters())
    table = [(p.numel(), (i % 2) if every_other else 0) for i, p in enumerate(params)]
    flat = _Flat(table, dev, [p.detach().cpu().numpy().ravel() for p in params])
    for p, v in zip(params, flat.views):
        p.data = v.view_as(p)
    return flat


def test_model_on_misaligned_parameters_meets_the_float64_bounds(dev, world, hidden, parity_report):
    """sage_model_cases' M2 (three blocks, 40 -> 48, the vector-layout twins and k_gemm_dual when everything is aligned) with its parameters
    re-pointed into one flat buffer, every other one at an odd element offset, trained three steps with optim.Adam(max_grad_norm=0.5) in
    deterministic mode.

    Bit equality with the same model in aligned storage was the first form of this test and cannot hold: the scalar and the 16-byte form
    of two kernels inline the same expression but are contracted differently by the compiler (in k_bn_apply<4, true>
    g - c1 - xhat c2 ends in one v_fma_f32, in k_bn_apply<1, true> the product is rounded by a v_pk_mul_f32 first; in k_adam
    beta2 v + (1 - beta2) g g is one v_pk_fma_f32 in the 16-byte loop, two products and a v_add_f32 in the scalar loop), so the first
    gradients already differ in the last bit.  Both roundings are legitimate, so the model on misaligned parameters is held to what the
    aligned one is held to (tests/test_sage_model_gpu.py): logits, hidden outputs, loss, gradients and running statistics of steps 1 and
    3 within FACTOR times the float32 restatement's error of the float64 model, the ReLU pattern exact outside the gate, and every
    parameter after every step within sage_model_cases.adam_reference's bound of the float64 step from its own pre-step state."""
    import test_sage_model_gpu as tm
    from graphpope_amd import sage
    from graphpope_amd.optim import Adam
    case, sampler, feats_cpu, feats, labels = world("M2")
    model = mc.case_model(case).to(dev).train()
    flat = _repoint(model, dev, every_other=True)
    named = list(model.named_parameters())
    assert sum(p.data_ptr() % 16 != 0 for _, p in named) == len(named) // 2
    n_hidden = len(case.sizes) - 1
    seeds, y = torch.as_tensor(mc.case_seeds(case), device=dev), labels.to(dev)
    lr, (b1, b2), eps = 0.01, (0.9, 0.999), 1e-8
    opt = Adam(model.parameters(), lr=lr, betas=(b1, b2), eps=eps, max_grad_norm=0.5)
    host = lambda t: t.detach().cpu().numpy().copy()
    worst = 0.0
    with sage.deterministic():
        n_id, adjs = sampler.sample(seeds, seed=case.sample_seed)
        batch = tm._read_batch(n_id, adjs)
        assert tm._same_batch(batch, mc.host_batch(case))
        x = sage.IndexedFeatures(feats, n_id)
        for step in range(1, 4):
            state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
            moments = [(host(opt.state[p]["exp_avg"]), host(opt.state[p]["exp_avg_sq"])) if "exp_avg" in opt.state[p]
                       else (np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32)) for _, p in named]
            del hidden[:]
            opt.zero_grad(set_to_none=True)
            torch.manual_seed(tm.MANUAL_SEED + step)
            logits = model(x, adjs)
            loss = sage.cross_entropy(logits, y)
            loss.backward()
            torch.cuda.synchronize()
            if step in (1, 3):
                got = tm._collect(model, logits, loss, [h[0] for h in hidden], batch[1])
                inp = mc.Inputs(state, feats_cpu[torch.from_numpy(batch[0])], batch[1], labels, mc.drawn_seeds(tm.MANUAL_SEED + step, n_hidden), 0)
                tm._judge("M2-misaligned-parameters-step-%d" % step, inp, got, parity_report)
            opt.step()
            torch.cuda.synchronize()
            coef = np.float32(opt.clip_coef.item())
            for (key, p), (m0, v0) in zip(named, moments):
                if p.grad is None:
                    assert np.array_equal(host(p), state[key].numpy()), key
                    continue
                want, bound = mc.adam_reference(state[key].numpy(), host(p.grad), m0, v0, coef, lr, b1, b2, eps, step)
                ratio = cases.worst_ratio(host(p), want, bound)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (step, key, ratio)
                assert np.abs(host(p) - state[key].numpy()).max() > 0, (step, key, "the step moved nothing")
    assert not sage.is_deterministic() and flat.untouched()
    print("M2 on misaligned parameters, Adam: worst error / bound %.3f" % worst)


# ---- pairwise -------------------------------------------------------------------------------------------------------------------
_PAIRWISE = [(row, name, 1) for row in cases.PAIRWISE_GPU_ROWS for name in cases.PAIRWISE_GPU_BITS if not (name == "A" and row[5])]
_PAIRWISE += [((257, 128, 256, 8, 1, 0, 0), "X", 2)]


@pytest.mark.parametrize("row,operand,off", _PAIRWISE, ids=["n%d_d%d_k%d_f%d_x%d_id%d-%s-off%d" % (r[:6] + (o, f)) for r, o, f in _PAIRWISE])
def test_pairwise_with_a_misaligned_operand(row, operand, off, dev, lib):
    """pope_pairwise_features / _by_id with X, A, x or out misaligned (the scratch holds float2 pairs, so 4 bytes is below what it may be
    given: that bit stays with the CPU table): the assertion of test_pairwise_plan_gpu.py against want64 -- 1e-5 absolute on the scaled
    values, exact zeros at the coincident pair -- and the feature columns equal x bit for bit."""
    from graphpope_amd import _lib
    n, d, k, f, has_x, by_id, knob = row
    assert knob == 0 and has_x
    mask = cases.PAIRWISE_GPU_BITS[operand]
    assert _name(lib.pope_pairwise_kernel_name_at, n, d, k, f, has_x, by_id, _cus(dev), mask) == cases.PAIRWISE[row][mask]
    assert _name(lib.pope_pairwise_kernel_name_at, n, d, k, f, has_x, by_id, _cus(dev), 0) == pw.CASES[row] != cases.PAIRWISE[row][mask]
    emb, anchors = pw.inputs(n, d, k)
    x = pc.features(n, f)
    o = lambda name: off if name == operand else 0
    t = {"X": misaligned.place(np.array(emb), dev, o("X")), "x": misaligned.place(x, dev, o("x"))}
    if not by_id:
        t["A"] = misaligned.place(emb[anchors], dev, o("A"))
    ids_d = torch.from_numpy(np.array(anchors, dtype=np.int64)).to(dev)
    sbytes = (lib.pope_pairwise_by_id_scratch_bytes if by_id else lib.pope_pairwise_scratch_bytes)(n, k, d)
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
    assert scratch.data_ptr() % 16 == 0
    for fn in pc.FNS:
        t["out"] = misaligned.place(np.full((n, f + k), SENTINEL), dev, o("out"))
        assert t[operand].data_ptr() % 16 == 4 * off
        p = _lib.ptr
        if by_id:
            _lib.check(lib.pope_pairwise_features_by_id(p(t["x"]), f, p(t["X"]), n, d, p(ids_d), k, _lib.METRIC[fn], p(t["out"]), f + k, f, p(scratch),
                                                        sbytes, _stream()))
        else:
            _lib.check(lib.pope_pairwise_features(p(t["x"]), f, p(t["X"]), n, d, p(t["A"]), k, _lib.METRIC[fn], p(t["out"]), f + k, f, p(scratch), sbytes,
                                                  _stream()))
        torch.cuda.synchronize()
        out = t["out"].cpu().numpy()
        tag = (row, operand, off, fn)
        assert np.array_equal(out[:, :f].view(np.uint32), x.view(np.uint32)), tag
        got, want = out[:, f:], pw.want64(n, d, k, fn)
        assert np.isfinite(got).all(), tag
        err = float(np.abs(got - want).max())
        print("%s: max error %.3g" % (tag, err))
        assert err <= 1e-5, tag
        if fn == "euclidean":
            assert got[5, 0] == 0.0 and got[7, 0] == 0.0, tag
        _assert_guards(t, tag)


# ---- geodesic -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_planes(dev):
    import os
    from graphpope_amd import engine
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geodesic_rmat11_seed42.npz"))
    n, k, f = cases.FINALIZE_SHAPE
    assert int(g["num_nodes"]) == n
    csr = engine.build_csr(torch.as_tensor(g["edge_index"].astype(np.int64), device=dev), n)
    anchors = np.random.RandomState(42).choice(n, size=k, replace=False)
    hp = engine.bfs(csr, anchors)
    x = np.random.RandomState(1).rand(n, f).astype(np.float32)
    return hp, x


@pytest.mark.parametrize("operand,off", [("x", 1), ("out", 1), ("out", 2)])
def test_finalize_with_a_misaligned_operand(operand, off, golden_planes, dev, lib):
    """pope_geodesic_finalize on the rmat11 golden graph at F = 8, K = 64 with x, then out, misaligned: k_finalize<false>, and every value
    (one IEEE division each, and the copied features) has the bits of the aligned call."""
    from graphpope_amd import engine
    hp, x = golden_planes
    n, k, f = cases.FINALIZE_SHAPE
    mask = 1 if operand == "x" else 2
    assert _name(lib.pope_finalize_kernel_name_at, n, k, f, 1, 1, mask) == cases.FINALIZE[(1, mask)] == "k_finalize<false>"
    assert _name(lib.pope_finalize_kernel_name_at, n, k, f, 1, 1, 0) == cases.FINALIZE[(1, 0)]
    outs = []
    for o in (0, off):
        t = {"x": misaligned.place(x, dev, o if operand == "x" else 0), "out": misaligned.place(np.full((n, f + k), SENTINEL), dev, o if operand == "out" else 0)}
        assert t[operand].data_ptr() % 16 == 4 * o
        engine.finalize(hp.valid(), hp.n_hop_bits, n, k, t["x"], f, t["out"])
        torch.cuda.synchronize()
        _assert_guards(t, (operand, o))
        outs.append(t["out"].clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert np.array_equal(outs[1][:, :f].cpu().numpy().view(np.uint32), x.view(np.uint32)) and bool((outs[1][:, f:] != SENTINEL).all())


@pytest.mark.parametrize("operand", ["x", "out"])
def test_concat_with_a_misaligned_operand(operand, dev):
    from graphpope_amd import engine
    n, f, cols = 257, 8, 24
    x = np.random.RandomState(2).rand(n, f).astype(np.float32)
    t = {"x": misaligned.place(x, dev, 1 if operand == "x" else 0), "out": misaligned.place(np.full((n, cols), SENTINEL), dev, 1 if operand == "out" else 0)}
    engine.copy_features(t["x"], f, t["out"])
    torch.cuda.synchronize()
    out = t["out"].cpu().numpy()
    assert np.array_equal(out[:, :f].view(np.uint32), x.view(np.uint32)) and (out[:, f:] == SENTINEL).all()
    _assert_guards(t, operand)


@pytest.mark.parametrize("build", ["build_csr", "build_csr_canonical"])
def test_csr_builds_from_an_edge_list_that_is_8_byte_aligned(build, dev):
    """src and dst one int64 into their buffer (8-byte, not 16-byte aligned; E even): one edge per lane instead of pairs, the same rowptr
    and col as from an aligned copy."""
    from graphpope_amd import engine, synth
    n = 2000
    ei = np.asarray(synth.powerlaw_graph(n, 12000, seed=3, alpha=0.9, shift=0.8)).astype(np.int64)
    ei = ei[:, :ei.shape[1] // 2 * 2]
    e = ei.shape[1]
    assert e % 2 == 0 and e > 4000
    buf = torch.full((2 * e + 2,), -1, dtype=torch.int64, device=dev)
    view = buf[1:1 + 2 * e].view(2, e)
    view.copy_(torch.from_numpy(ei))
    assert view[0].data_ptr() % 16 == 8 and view[1].data_ptr() % 16 == 8
    aligned = torch.from_numpy(ei).to(dev)
    assert aligned.data_ptr() % 16 == 0
    a, b = getattr(engine, build)(aligned, n), getattr(engine, build)(view, n)
    torch.cuda.synchronize()
    assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col[:e], b.col[:e]) and torch.equal(a.erow[:e], b.erow[:e])
    assert int(buf[0]) == -1 and int(buf[-1]) == -1 and torch.equal(view.cpu(), torch.from_numpy(ei))
