"""The table of tests/test_workspace_gpu.py: one row per (entry point that takes a caller-owned scratch, layout branch of that scratch).
Not a test module.

A row builds its operands and its expected outputs from the case modules the entry point's own tests use -- sage_backward_cases (PATHS,
FORWARD, ForwardReference, the exact family), deterministic_cases, bn_epilogue_cases, pairwise_plan_cases.CASES, node2vec_det_cases,
logreg_cases, the constructed graphs of test_sampler_gpu.py, the level-table graph of test_geodesic_gpu.py, the star with pendant paths
of test_anchor_select_gpu.py, the goldens and the CPU oracle -- and compares as those tests compare: no reference is derived here.  Each
shape is the smallest of its module that reaches the branch named beside it.

Row.make(dev, lib) returns a Call:
    need                  what the size query answers for the call's arguments (asked under the row's knobs and mode)
    run(ptr, nbytes)      the library call on (ptr, nbytes) as its scratch, synchronised; returns the library's code
    reset()               inputs that the call overwrites and outputs back to their state before a call (outputs: a sentinel)
    outputs()             {name: host array} of everything the call promises -- the valid prefixes only where the header leaves the
                          rest unspecified
    check(outputs)        against the row's reference
    untouched()           every output still holds what reset() put there
    guards                further GuardedScratch buffers the call writes (the CSR builds' aux, col and erow)
    refusal / null_refusal   the code include/graphpope_hip.h documents for a scratch that is too small / NULL; runs_with_less marks
                          the documented exception, sage_conv_forward*: told how much scratch there is, forward_plan avoids stream-K
                          when the slabs do not fit, so less scratch gives the same result by other kernels

Every knob or mode a row sets is set by Row.context and restored in its `finally`.
`weight` orders the rows of one entry point by scratch size: the heaviest other row is the one whose leftovers a row's `keep` run finds."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import torch

import bn_epilogue_cases as bn
import deterministic_cases as det_cases
import logreg_cases
import node2vec_det_cases as n2v_cases
import pairwise_cases as pc
import pairwise_plan_cases as pw_cases
import sage_backward_cases as sb
from conftest import GOLDEN, load_golden
from workspace import GuardedScratch

ERR_INVALID, ERR_WORKSPACE = -1, -5
I_SENTINEL = -7
PROPS = ("contained", "self_initialising", "refused")


def _p(t):
    from graphpope_amd import _lib
    return _lib.ptr(t)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _to(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


class _At:
    """Stands in for a tensor where a helper of another test module calls .data_ptr() on the scratch it is given."""

    def __init__(self, ptr):
        self.addr = ptr.value or 0

    def data_ptr(self):
        return self.addr


class Call:
    entry = ""
    need = 0
    refusal = ERR_WORKSPACE
    null_refusal = ERR_INVALID                   # POPE_ERR_INVALID: "bad argument (null pointer, ...)"
    runs_with_less = False
    guards = ()

    def reset(self):
        raise NotImplementedError

    def run(self, ptr, nbytes):
        raise NotImplementedError

    def outputs(self):
        raise NotImplementedError

    def check(self, out):
        raise NotImplementedError

    def untouched(self):
        raise NotImplementedError


class Row:
    def __init__(self, entry, name, make, weight, knobs=(), det=False, props=PROPS, branch=""):
        self.entry, self.name, self.make, self.weight, self.knobs, self.det, self.props, self.branch = entry, name, make, weight, knobs, det, props, branch
        self.id = "%s-%s" % (entry, name)

    @contextlib.contextmanager
    def context(self, lib):
        """The row's knobs (name in graphpope_amd._lib, value, value to restore) and the deterministic mode, for the length of the block."""
        from graphpope_amd import _lib
        assert lib.sage_get_deterministic() == 0, "an earlier test left the switch on"
        try:
            for knob, value, _ in self.knobs:
                _lib.check(lib.pope_debug_set(getattr(_lib, knob), value))
            if self.det:
                lib.sage_set_deterministic(1)
            yield
        finally:
            lib.sage_set_deterministic(0)
            for knob, _, default in self.knobs:
                lib.pope_debug_set(getattr(_lib, knob), default)


ROWS = []


def _row(entry, name, make, weight, **kw):
    ROWS.append(Row(entry, name, make, weight, **kw))


def donor_of(row):
    """The heaviest other row of the same entry point (None if the row is alone): a different, larger call whose leftovers the `keep`
    run starts from; the heaviest row itself takes the second heaviest."""
    others = [r for r in ROWS if r.entry == row.entry and r is not row]
    return max(others, key=lambda r: r.weight) if others else None


# =====================================================================================================================================
# SAGE backward: sage_conv_backward, sage_conv_backward_indexed (sage_backward_cases.PATHS: one shape per layout family)
# =====================================================================================================================================
class BackwardCall(Call):
    def __init__(self, dev, lib, case, det=False):
        import test_sage_backward_gpu as bwd
        self.lib, self.case, self.bwd = lib, case, bwd
        self.entry = "sage_conv_backward_indexed" if case["indexed"] else "sage_conv_backward"
        name = bwd._backward_name(lib, case, dev)
        if det:
            assert "k_scatter_sum_det" in name and "k_scatter_mean" not in name, name
        else:
            assert name == sb.expected_name(case["shape"], case["extra"], case["grad_x"], case["grad_b"], case["xcd"]), name
        self.ref = sb.reference(case, case["shape"][0])
        self.ref.assert_exact_family_is_exact()                  # atomic sums in any order give the same bits
        self.b = bwd.Buffers(case, dev, self.ref.nnz)            # (sized under the row's mode: the query includes the index's room)
        self.need = self.b.scratch_bytes
        self.b.scratch = None
        self.b.load(self.ref, extents=False)
        self.outs = [t for t in (self.b.grad_x, self.b.grad_w_l, self.b.grad_w_r, self.b.grad_b) if t is not None]
        self.got = None

    def reset(self):
        for t in self.outs:
            t.fill_(sb.SENTINEL)

    def run(self, ptr, nbytes):
        from graphpope_amd import _lib
        self.b.scratch, self.b.scratch_bytes = (None if ptr is None else _At(ptr)), nbytes
        try:
            self.got = self.b.run(self.lib)
        except _lib.PopeError as e:
            return e.code
        return 0

    def outputs(self):
        return self.got

    def check(self, out):
        self.bwd._check(self.case, self.ref, out, self.case["id"])

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == sb.SENTINEL).all()) for t in self.outs)


def _backward(shape, extra=300, det=False, **kw):
    case = sb._case(shape, extra, **kw)
    return lambda dev, lib: BackwardCall(dev, lib, case, det)


for _shape, _branch in (((4065, 256, 256), "streamk_xcd"), ((1700, 260, 260), "streamk"), ((1030, 40, 24), "dual"),
                        ((515, 37, 30), "twin with splits"), ((256, 64, 64), "twin without splits")):
    _row("sage_conv_backward", "%dx%d-%d" % _shape, _backward(_shape), int(np.prod(_shape)), branch=_branch)
for _shape in ((1030, 40, 24), (515, 37, 30)):
    _row("sage_conv_backward", "%dx%d-%d-det" % _shape, _backward(_shape, det=True), int(np.prod(_shape)), det=True,
         branch="the inverted index of the deterministic sum behind the layout")
_row("sage_conv_backward_indexed", "2100x756-256-nogx", _backward((2100, 756, 256), grad_x=False, indexed=True), 2100 * 756 * 256,
     branch="streamk_xcd through n_id")
_row("sage_conv_backward_indexed", "1030x40-24-nogx", _backward((1030, 40, 24), grad_x=False, indexed=True), 1030 * 40 * 24,
     branch="k_gather_rows builds the destination rows in the scratch")


# =====================================================================================================================================
# SAGE forward: the four entry points (sage_backward_cases.FORWARD / ForwardReference, as test_sage_backward_gpu.py calls them)
# =====================================================================================================================================
class ForwardCall(Call):
    """`cap` destinations at the capacity of the buffers; n_true < cap: `dims` on the device, the scratch still sized for the capacity.
    x_dst: "given" / "null" (indexed only: the rows matrix then lives in the scratch tail at align_up(forward bytes, 256))."""

    def __init__(self, dev, lib, shape, name, indexed=False, x_dst="given", stats=False, n_true=None):
        from graphpope_amd import _lib
        cap, c_in, c_out = shape
        self.lib, self.shape, self.indexed, self.stats, self.null_x_dst = lib, shape, indexed, stats, indexed and x_dst == "null"
        self.entry = "sage_conv_forward" + ("_indexed" if indexed else "") + ("_stats" if stats else "")
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        buf = ctypes.create_string_buffer(96)
        _lib.check(lib.sage_forward_kernel_name(cap, c_in, c_out, cus, buf, 96))
        assert buf.value.decode() == name, buf.value
        self.extents = n_true is not None
        n = self.n = n_true if self.extents else cap
        ref = self.ref = sb.forward_reference(n, c_in, c_out)
        ref.assert_exact_family_is_exact()
        n_src_cap, self.n_rows = cap + sb.FORWARD_EXTRA, cap + sb.FORWARD_EXTRA + 500
        self.n_src_cap = n_src_cap
        self.nnz_cap = ref.nnz + (64 if self.extents else 0)
        rs = np.random.RandomState(n)
        rowptr, col = sb.padded_csr(ref.rowptr, ref.col, cap, self.nnz_cap, ref.n_src, n_src_cap, rs)
        if indexed:
            feats, n_id = sb.indexed_rows(ref.x, self.n_rows, n_src_cap, c_in, rs)
            self.n_id = _to(n_id, dev)
        else:
            feats = sb.nan_padded(ref.x, n_src_cap)
        self.x, self.rowptr, self.col = _to(feats, dev), _to(rowptr, dev), _to(col, dev)
        self.w_l, self.w_r, self.b = _to(ref.w_l, dev), _to(ref.w_r, dev), _to(ref.b, dev)
        self.dims = torch.tensor([n, ref.n_src, ref.nnz, 0], dtype=torch.int32, device=dev) if self.extents else None
        f = lambda *s: torch.empty(*s, device=dev)
        self.agg, self.out, self.x_dst = f(cap, c_in), f(cap, c_out), (f(cap, c_in) if indexed and not self.null_x_dst else None)
        self.parts_cap = (cap + 15) // 16
        self.pa, self.pb = (torch.empty((self.parts_cap, c_out), dtype=torch.float64, device=dev) for _ in range(2)) if stats else (None, None)
        self.info = (ctypes.c_int32 * 2)(0, 0)
        self.need = (lib.sage_conv_forward_indexed_scratch_bytes if self.null_x_dst else lib.sage_conv_forward_scratch_bytes)(cap, c_in, c_out)
        if self.null_x_dst:
            up = lambda v: (v + 255) // 256 * 256
            assert self.need == up(lib.sage_conv_forward_scratch_bytes(cap, c_in, c_out)) + up(cap * c_in * 4)
            self.null_refusal = ERR_WORKSPACE                      # "without x_dst the scratch must hold ..."
        else:
            self.runs_with_less = True

    def reset(self):
        for t in (self.agg, self.out, self.x_dst, self.pa, self.pb):
            if t is not None:
                t.fill_(sb.SENTINEL)
        self.info[0] = self.info[1] = I_SENTINEL

    def run(self, ptr, nbytes):
        cap, c_in, c_out = self.shape
        n_dst, nnz = (cap, self.nnz_cap) if self.extents else (self.n, self.ref.nnz)
        if self.indexed:
            args = (_p(self.rowptr), _p(self.col), _p(self.n_id), self.n_src_cap, n_dst, nnz, _p(self.x), self.n_rows, c_in, _p(self.w_l), _p(self.b),
                    _p(self.w_r), c_out, _p(self.agg), _p(self.x_dst), _p(self.out), ptr, nbytes, _p(self.dims))
            fn = self.lib.sage_conv_forward_indexed_stats if self.stats else self.lib.sage_conv_forward_indexed
        else:
            args = (_p(self.rowptr), _p(self.col), self.n_src_cap, n_dst, nnz, _p(self.x), c_in, _p(self.w_l), _p(self.b), _p(self.w_r), c_out,
                    _p(self.agg), _p(self.out), ptr, nbytes, _p(self.dims))
            fn = self.lib.sage_conv_forward_stats if self.stats else self.lib.sage_conv_forward
        rc = fn(*args, _p(self.pa), _p(self.pb), self.parts_cap, self.info, _stream()) if self.stats else fn(*args, _stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        out = {"agg": self.agg.cpu().numpy(), "out": self.out.cpu().numpy()}
        if self.x_dst is not None:
            out["x_dst"] = self.x_dst.cpu().numpy()
        if self.stats:
            tiles = max(int(self.info[0]), 0)
            out.update(info=np.array(list(self.info)), pa=self.pa.cpu().numpy()[:tiles], pb=self.pb.cpu().numpy()[:tiles])
        return out

    def check(self, out):
        n, ref = self.n, self.ref
        want = [("agg", ref.agg), ("out", ref.out)] + ([("x_dst", ref.x[:n].astype(np.float64))] if "x_dst" in out else [])
        for what, w in want:
            got = out[what].astype(np.float64)
            assert np.array_equal(got[:n], w), (what, int((got[:n] != w).sum()))
            assert np.array_equal(got[n:], np.full_like(got[n:], sb.SENTINEL)), (what, "rows past the true count were written")
        if self.stats:
            tiles, rpp = int(out["info"][0]), int(out["info"][1])
            assert tiles > 0 and rpp > 0 and tiles <= self.parts_cap and tiles * rpp >= n, (tiles, rpp)
            # exact family: every out value is a multiple of 2^-7 below 2^17, so the float64 sums of a tile's values and squares are exact
            for t in range((n + rpp - 1) // rpp):
                tile = ref.out[t * rpp:min((t + 1) * rpp, n)]
                assert np.array_equal(out["pa"][t], tile.sum(axis=0)) and np.array_equal(out["pb"][t], (tile * tile).sum(axis=0)), t

    def untouched(self):
        torch.cuda.synchronize()
        ts = [t for t in (self.agg, self.out, self.x_dst, self.pa, self.pb) if t is not None]
        return all(bool((t == sb.SENTINEL).all()) for t in ts) and self.info[0] == I_SENTINEL


def _forward(shape, name, **kw):
    return lambda dev, lib: ForwardCall(dev, lib, shape, name, **kw)


_FORMS = {"streamk": 0, "overlapped": 3, "tile16": 4, "plain": 7}              # rows of sage_backward_cases.FORWARD
for _form, _i in _FORMS.items():
    _shape, _knob, _name = sb.FORWARD[_i]
    _knobs = ((_knob, 0, 1),) if _knob else ()
    for _indexed in (False, True):
        _row("sage_conv_forward_indexed" if _indexed else "sage_conv_forward", "%dx%d-%d-%s" % (_shape + (_form,)),
             _forward(_shape, _name, indexed=_indexed), int(np.prod(_shape)), knobs=_knobs, branch=_name)
_S4160, _S5800, _S515 = sb.FORWARD[0], sb.FORWARD[3], sb.FORWARD[7]
_row("sage_conv_forward_indexed", "4160x256-256-streamk-no_x_dst", _forward(_S4160[0], _S4160[2], indexed=True, x_dst="null"), 4160 * 256 * 256 + 1,
     branch="the rows matrix in the scratch tail behind the slabs")
_row("sage_conv_forward_indexed", "515x37-30-plain-no_x_dst", _forward(_S515[0], _S515[2], indexed=True, x_dst="null"), 515 * 37 * 30 + 1,
     branch="the rows matrix at offset 0 (no slabs)")
_row("sage_conv_forward", "4160x256-256-streamk-true4129", _forward(_S4160[0], _S4160[2], n_true=4160 - 31), 4160 * 256 * 256 - 1,
     branch="dims on the device, scratch sized for the capacity")
_row("sage_conv_forward_stats", "5800x256-256-overlapped", _forward(_S5800[0], _S5800[2], stats=True), 5800 * 256 * 256, branch=_S5800[2])
_row("sage_conv_forward_indexed_stats", "5800x256-256-overlapped", _forward(_S5800[0], _S5800[2], indexed=True, stats=True), 5800 * 256 * 256,
     branch=_S5800[2])


# =====================================================================================================================================
# sage_scatter_mean_det (deterministic_cases: the hand-built block, the random blocks under a capacity)
# =====================================================================================================================================
class ScatterDetCall(Call):
    entry = "sage_scatter_mean_det"
    refusal = ERR_INVALID

    def __init__(self, dev, lib, c, true=None):
        import test_deterministic_gpu as tdet
        self.lib, self.c = lib, c
        cap_dst, cap_src = det_cases.N_DST, det_cases.N_SRC
        if true is None:
            rowptr, col = det_cases.hand_built_block()
            n_dst, n_src = cap_dst, cap_src
            self.nnz, self.dims = len(col), None
        else:
            n_dst, n_src = true
            rowptr, col = det_cases.random_block(n_dst, n_src, seed=n_dst)
            assert np.bincount(col, minlength=n_src).max() > 64
        gagg, gx = tdet._inputs(c, n_dst, n_src, seed=n_dst + c)
        self.want = det_cases.scatter_mean_reference(rowptr, col, n_src, n_dst, gagg, gx)
        self.n_src = n_src
        if true is not None:                                          # everything at the capacity, poison past the true sizes
            self.nnz = len(col) + 64
            self.dims = torch.tensor([n_dst, n_src, len(col), 0], dtype=torch.int32, device=dev)
            rowptr, col = sb.padded_csr(rowptr, col, cap_dst, self.nnz, n_src, cap_src, np.random.RandomState(n_dst))
            gagg = sb.nan_padded(gagg, cap_dst)
            full = np.full((cap_src, c), sb.SENTINEL, dtype=np.float32)
            full[:n_dst] = gx[:n_dst]
            gx = full
        self.gx0 = gx
        self.rowptr, self.col, self.gagg, self.gx = _to(rowptr, dev), _to(col, dev), _to(gagg, dev), _to(gx, dev)
        self.need = lib.sage_scatter_mean_det_scratch_bytes(cap_src, cap_dst, self.nnz)

    def reset(self):
        self.gx.copy_(torch.from_numpy(self.gx0))

    def run(self, ptr, nbytes):
        rc = self.lib.sage_scatter_mean_det(_p(self.rowptr), _p(self.col), det_cases.N_SRC, det_cases.N_DST, self.nnz, _p(self.gagg), self.c,
                                            _p(self.gx), ptr, nbytes, _p(self.dims), _stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return {"grad_x": self.gx.cpu().numpy()}

    def check(self, out):
        got = out["grad_x"]
        assert np.array_equal(got[:self.n_src].view(np.int32), self.want.view(np.int32)), int((got[:self.n_src].view(np.int32) != self.want.view(np.int32)).sum())
        assert np.array_equal(got[self.n_src:], np.full_like(got[self.n_src:], sb.SENTINEL)), "rows past the true sources were written"

    def untouched(self):
        return np.array_equal(self.gx.cpu().numpy().view(np.int32), self.gx0.view(np.int32))


for _c in (256, 37):
    _row("sage_scatter_mean_det", "hand_built-c%d" % _c, lambda dev, lib, c=_c: ScatterDetCall(dev, lib, c), 1000 + _c,
         branch="lists of 0, 1, 2, 64, 65 and 129 entries")
_row("sage_scatter_mean_det", "true100x170-of-130x200-c37", lambda dev, lib: ScatterDetCall(dev, lib, 37, true=(100, 170)), 2000,
     branch="device extents, index sized for the capacity")
_row("sage_scatter_mean_det", "true40x90-of-130x200-c256", lambda dev, lib: ScatterDetCall(dev, lib, 256, true=(40, 90)), 1500,
     branch="device extents, index sized for the capacity")


# =====================================================================================================================================
# BatchNorm + ReLU + dropout: the four calls (bn_epilogue_cases: _make, reference, check)
# =====================================================================================================================================
class BnCall(Call):
    """One forward + backward pair of a training-mode case, as bn_epilogue_cases.check takes it; the call under test gets the scratch
    of the row, its companion a buffer of its own."""

    def __init__(self, dev, lib, m, c, which):
        self.lib, self.dev, self.which = lib, dev, which
        self.entry = {"forward": "sage_bn_relu_dropout_forward", "forward_stats": "sage_bn_relu_dropout_forward_stats",
                      "backward": "sage_bn_relu_dropout_backward", "backward_bias": "sage_bn_relu_dropout_backward_bias"}[which]
        self.case = bn._make("(%d, %d) train p=0.5" % (m, c), m, c, True, 0.5, ext_rows_per_part=16 if which == "forward_stats" else None)
        self.ref = bn.reference(self.case)
        self.need = lib.sage_bn_scratch_bytes(c)
        self.own = torch.empty(self.need, dtype=torch.uint8, device=dev)
        self.partials = [torch.as_tensor(a, device=dev) for a in bn.external_partials(self.case)] if which == "forward_stats" else None
        self.reset()

    def reset(self):
        import test_bn_epilogue_f64_gpu as tbn
        t = self.t = tbn._forward_args(self.case, self.dev)
        for k in ("mean", "rstd", "gg", "gb"):
            t[k].fill_(float(bn.SENTINEL))
        self.cs = torch.full((self.case.x.shape[1],), float(bn.SENTINEL), device=self.dev)

    def _forward(self, ptr, nbytes):
        case, t = self.case, self.t
        cap, c = case.x.shape
        head = (_p(t["x"]), cap, c, _p(t["gamma"]), _p(t["beta"]), _p(t["rm"]), _p(t["rv"]), _p(t["nbt"]), bn.MOMENTUM, bn.EPS, 1, case.p,
                case.seed, _p(t["y"]), _p(t["mean"]), _p(t["rstd"]), ptr, nbytes, None, None)
        if self.which == "forward_stats":
            pa, pb = self.partials
            return self.lib.sage_bn_relu_dropout_forward_stats(*head, _p(pa), _p(pb), pa.shape[0], case.ext_rows_per_part, _stream())
        return self.lib.sage_bn_relu_dropout_forward(*head, _stream())

    def _backward(self, ptr, nbytes):
        case, t = self.case, self.t
        cap, c = case.x.shape
        args = (_p(t["x"]), _p(t["dy"]), cap, c, _p(t["gamma"]), _p(t["beta"]), _p(t["mean"]), _p(t["rstd"]), 1, case.p, case.seed, _p(t["gx"]),
                _p(t["gg"]), _p(t["gb"]), ptr, nbytes, None, None)
        if self.which == "backward_bias":
            return self.lib.sage_bn_relu_dropout_backward_bias(*args, _p(self.cs), _stream())
        return self.lib.sage_bn_relu_dropout_backward(*args, _stream())

    def run(self, ptr, nbytes):
        own = (_p(self.own), self.need)
        under_test_first = self.which.startswith("forward")
        rc = self._forward(ptr, nbytes) if under_test_first else self._forward(*own)
        if rc == 0:
            rc = self._backward(*own) if under_test_first else self._backward(ptr, nbytes)
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        host = {k: None if v is None else v.cpu().numpy() for k, v in self.t.items()}
        out = {"save_mean": host["mean"], "save_rstd": host["rstd"], "running_mean": host["rm"], "running_var": host["rv"], "y": host["y"],
               "grad_x": host["gx"], "grad_beta": host["gb"], "grad_gamma": host["gg"], "num_batches_tracked": host["nbt"]}
        if self.which == "backward_bias":
            out["grad_x_colsum"] = self.cs.cpu().numpy()
        return out

    def check(self, out):
        bn.check(self.case, self.ref, out)
        assert int(out["num_batches_tracked"][0]) == 1
        if self.which == "backward_bias":          # the comparison of test_epilogue_gpu.py: against the float64 column sums of the grad_x the call wrote
            gx = out["grad_x"].astype(np.float64)
            assert np.abs(out["grad_x_colsum"].astype(np.float64) - gx.sum(axis=0)).max() <= 1e-6 * np.abs(gx).sum(axis=0).max()

    def untouched(self):
        t, s = self.t, float(bn.SENTINEL)
        torch.cuda.synchronize()
        if self.which.startswith("forward"):
            same = all(np.array_equal(t[k].cpu().numpy(), w) for k, w in (("rm", self.case.running_mean), ("rv", self.case.running_var)))
            return same and int(t["nbt"]) == 0 and all(bool((t[k] == s).all()) for k in ("y", "mean", "rstd"))
        return all(bool((v == s).all()) for v in (t["gx"], t["gg"], t["gb"], self.cs))


for _which in ("forward", "forward_stats", "backward", "backward_bias"):
    for _m, _c in ((2, 5), (37, 10), (513, 260)):
        _row("sage_bn_relu_dropout_" + _which, "%dx%d" % (_m, _c), lambda dev, lib, m=_m, c=_c, w=_which: BnCall(dev, lib, m, c, w), _m * _c,
             branch="scalar columns" if _c % 4 else "16-byte columns, a second column block")


# =====================================================================================================================================
# The fan-out sampler: four entry points (the constructed graphs of test_sampler_gpu.py, the CPU restatement oracle.sample_hop)
# =====================================================================================================================================
def _tail_graph(n):
    """test_sampler_gpu.test_tail_of_the_position_key_map_is_cleared: the last N & 3 nodes are the seeds and neighbours of node 0."""
    import test_sampler_gpu as ts
    tail = list(range(n - (n & 3), n))
    rows = {i: [i + 1 if i + 1 < n else 1] for i in range(1, n)}
    rows[0] = tail + [1]
    return ts._from_rows(rows, n) + (n, np.array(tail))


class SampleCall(Call):
    """form: "hop" (sage_sample_hop, one fan-out, -1 allowed), "batch" (sage_sample_batch), "device" (sage_sample_batch_device) or
    "epoch" (sage_sample_epoch_batch_device: the seeds are order[first .. first + T) and y_out = labels[seeds])."""
    SEED = 7

    def __init__(self, dev, lib, graph, sizes, form):
        self.lib, self.form, self.sizes = lib, form, [int(f) for f in sizes]
        self.entry = {"hop": "sage_sample_hop", "batch": "sage_sample_batch", "device": "sage_sample_batch_device",
                      "epoch": "sage_sample_epoch_batch_device"}[form]
        rowptr, col, n, seeds = graph
        rowptr, col, seeds = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(seeds, np.int64)
        self.n, self.t0, h = int(n), len(seeds), len(self.sizes)
        orc = _oracle()
        self.want, targets = [], seeds
        for hop, f in enumerate(self.sizes):
            rp, cl, ids = orc.sample_hop(rowptr, col, targets, f, self.SEED, hop)
            self.want.append((np.asarray(rp), np.asarray(cl), np.asarray(ids)))
            targets = np.asarray(ids, np.int64)
        self.rowptr = _to(rowptr.astype(np.int32), dev)
        self.col = _to(np.concatenate([col, np.zeros(1, np.int64)]).astype(np.int32), dev)      # (a graph without edges still needs an address)
        if form == "hop":
            assert h == 1
            deg = rowptr[seeds + 1] - rowptr[seeds]
            self.t_cap, self.caps = [self.t0], [int(deg.sum()) if self.sizes[0] < 0 else self.t0 * self.sizes[0]]
        else:
            assert all(f > 0 for f in self.sizes)
            self.t_cap, self.caps, t = [], [], self.t0
            for f in self.sizes:
                self.t_cap.append(t)
                self.caps.append(t * f)
                t += t * f
        self.need = lib.sage_sample_scratch_bytes(self.n, self.t_cap[-1], self.caps[-1])
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
        self.o_rowptr = [i32(tc + 1) for tc in self.t_cap]
        self.o_col = [i32(max(c, 1)) for c in self.caps]
        self.o_n_id = [torch.empty(tc + c, dtype=torch.int64, device=dev) for tc, c in zip(self.t_cap, self.caps)]
        self.dims = i32(4 * h).view(h, 4)
        self.nnz, self.n_src = (ctypes.c_int64 * h)(), (ctypes.c_int64 * h)()
        if form == "epoch":
            rs = np.random.RandomState(3)
            self.first = 5
            others = np.setdiff1d(np.arange(self.n), seeds)
            order = np.concatenate([rs.permutation(others)[:self.first], seeds, rs.permutation(others)[self.first:]])
            self.labels_host = rs.randint(0, 9, size=self.n).astype(np.int64)
            self.order, self.labels = _to(order.astype(np.int64), dev), _to(self.labels_host, dev)
            self.first_dev = torch.tensor([self.first], dtype=torch.int64, device=dev)
            self.y_out = torch.empty(self.t0, dtype=torch.int64, device=dev)
        else:
            self.seeds = _to(seeds, dev)
        self.seeds_host = seeds
        self.reset()

    def _all(self):
        return self.o_rowptr + self.o_col + self.o_n_id + [self.dims] + ([self.y_out] if self.form == "epoch" else [])

    def reset(self):
        for t in self._all():
            t.fill_(I_SENTINEL)
        for i in range(len(self.sizes)):
            self.nnz[i] = self.n_src[i] = I_SENTINEL

    def run(self, ptr, nbytes):
        lib, h = self.lib, len(self.sizes)
        arr = ctypes.c_void_p * h
        ptrs = lambda ts: arr(*[t.data_ptr() for t in ts])
        fan = (ctypes.c_int32 * h)(*self.sizes)
        if self.form == "hop":
            rc = lib.sage_sample_hop(_p(self.rowptr), _p(self.col), self.n, _p(self.seeds), self.t0, self.sizes[0], self.SEED, 0, _p(self.o_rowptr[0]),
                                     _p(self.o_col[0]), self.caps[0], _p(self.o_n_id[0]), self.nnz, self.n_src, ptr, nbytes, _stream())
        elif self.form == "batch":
            rc = lib.sage_sample_batch(_p(self.rowptr), _p(self.col), self.n, _p(self.seeds), self.t0, fan, h, self.SEED, ptrs(self.o_rowptr),
                                       ptrs(self.o_col), ptrs(self.o_n_id), self.nnz, self.n_src, ptr, nbytes, _stream())
        elif self.form == "device":
            rc = lib.sage_sample_batch_device(_p(self.rowptr), _p(self.col), self.n, _p(self.seeds), self.t0, fan, h, self.SEED, None,
                                              ptrs(self.o_rowptr), ptrs(self.o_col), ptrs(self.o_n_id), _p(self.dims), ptr, nbytes, _stream())
        else:
            rc = lib.sage_sample_epoch_batch_device(_p(self.rowptr), _p(self.col), self.n, _p(self.order), _p(self.first_dev), self.t0,
                                                    _p(self.labels), _p(self.y_out), fan, h, self.SEED, None, ptrs(self.o_rowptr), ptrs(self.o_col),
                                                    ptrs(self.o_n_id), _p(self.dims), ptr, nbytes, _stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        """The prefixes the header specifies: rows past n_dst are empty, entries past nnz / n_src are unspecified."""
        out, on_device = {}, self.form in ("device", "epoch")
        dims = self.dims.cpu().numpy()
        if on_device:
            out["dims"] = dims
        else:
            out["nnz"], out["n_src"] = np.array(list(self.nnz)), np.array(list(self.n_src))
        t = self.t0
        for i in range(len(self.sizes)):
            nnz, n_src = (int(dims[i, 2]), int(dims[i, 1])) if on_device else (int(self.nnz[i]), int(self.n_src[i]))
            ok = 0 <= nnz <= self.caps[i] and 0 <= n_src <= self.t_cap[i] + self.caps[i]
            rp = self.o_rowptr[i].cpu().numpy()
            out["rowptr%d" % i] = rp if on_device else rp[:t + 1]
            out["col%d" % i] = self.o_col[i].cpu().numpy()[:nnz if ok else 0]
            out["n_id%d" % i] = self.o_n_id[i].cpu().numpy()[:n_src if ok else 0]
            t = n_src if ok else 0
        if self.form == "epoch":
            out["y_out"] = self.y_out.cpu().numpy()
        return out

    def check(self, out):
        on_device = self.form in ("device", "epoch")
        t = self.t0
        for i, (rp, cl, ids) in enumerate(self.want):
            if on_device:
                assert out["dims"][i].tolist() == [t, len(ids), len(cl), 0], (i, out["dims"][i])
                got = out["rowptr%d" % i]
                assert np.array_equal(got[:t + 1], rp) and (got[t:] == len(cl)).all(), i
            else:
                assert (out["nnz"][i], out["n_src"][i]) == (len(cl), len(ids)), i
                assert np.array_equal(out["rowptr%d" % i], rp), i
            assert np.array_equal(out["col%d" % i], cl) and np.array_equal(out["n_id%d" % i], ids), i
            t = len(ids)
        if self.form == "epoch":
            assert np.array_equal(out["y_out"], self.labels_host[self.seeds_host])

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == I_SENTINEL).all()) for t in self._all()) and all(v == I_SENTINEL for v in list(self.nnz) + list(self.n_src))


def _sample(graph, sizes, form):
    return lambda dev, lib: SampleCall(dev, lib, graph(), sizes, form)


def _sampler_graph(which, *a):
    import test_sampler_gpu as ts
    return {"ring": ts._ring3_seeds, "big_row": ts._big_row}[which](*a)


_row("sage_sample_hop", "ring-T1023-f2", _sample(lambda: _sampler_graph("ring", 1023), (2,), "hop"), 1023, branch="count scan: one chain block, full")
_row("sage_sample_hop", "ring-T1024-f2", _sample(lambda: _sampler_graph("ring", 1024), (2,), "hop"), 1024, branch="count scan: entry T opens a second chain block")
_row("sage_sample_hop", "big_row-all", _sample(lambda: _sampler_graph("big_row"), (-1,), "hop"), 3000,
     branch="fan-out -1: cap + 1 crosses a 1024-item chain block (k_sample_all)")
_row("sage_sample_batch", "big_row-f25-10", _sample(lambda: _sampler_graph("big_row"), (25, 10), "batch"), 3000, branch="two hops: the regions alternate")
_row("sage_sample_batch", "ring-T16-f2-2", _sample(lambda: _sampler_graph("ring", 16), (2, 2), "batch"), 16, branch="two hops: the regions alternate")
_row("sage_sample_batch_device", "ring-T16-f2-2-2", _sample(lambda: _sampler_graph("ring", 16), (2, 2, 2), "device"), 4100,
     branch="three hops: map and state regions used and re-prepared")
for _n in (5, 6, 7):
    _row("sage_sample_batch_device", "tail-N%d-f4-4" % _n, _sample(lambda n=_n: _tail_graph(n), (4, 4), "device"), _n,
         branch="the map clear's N & 3 tail")
_row("sage_sample_epoch_batch_device", "ring-T16-f2-2", _sample(lambda: _sampler_graph("ring", 16), (2, 2), "epoch"), 16,
     branch="seeds through the device cursor, labels written by the first kernel")
_row("sage_sample_epoch_batch_device", "big_row-f25-10", _sample(lambda: _sampler_graph("big_row"), (25, 10), "epoch"), 3000,
     branch="a sampled row of 3 000 neighbours")


# =====================================================================================================================================
# CSR builds: pope_csr_build, pope_csr_build_canonical (scratch and aux; the expected CSR as test_geodesic_gpu.py states it)
# =====================================================================================================================================
def _csr_graph(e, n=50, hub=None, seed=0):
    """int64 [2, e] sorted by source with the edge list's own target order; hub = (node, edges of that node)."""
    rs = np.random.RandomState(seed + e)
    src = np.sort(rs.randint(0, n, size=e))
    if hub is not None:
        src[:hub[1]] = hub[0]
        src = np.sort(src)
    return np.stack([src, rs.randint(0, n, size=e)]).astype(np.int64), n


class CsrCall(Call):
    def __init__(self, dev, lib, ei, n, canonical=False, shuffled=False):
        self.lib, self.n, self.canonical = lib, n, canonical
        self.entry = "pope_csr_build_canonical" if canonical else "pope_csr_build"
        if shuffled:
            ei = ei[:, np.random.RandomState(1).permutation(ei.shape[1])]
            assert (np.diff(ei[0]) < 0).any()
        e = self.e = ei.shape[1]
        order = np.lexsort((ei[1], ei[0])) if (canonical or shuffled) else np.arange(e)
        self.want = {"rowptr": np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=n))]).astype(np.int32),
                     "col": ei[1][order].astype(np.int32), "erow": ei[0][order].astype(np.int32)}
        self.ei = _to(ei, dev)
        self.rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        slots = max(4, (e + 3) // 4 * 4)                             # "col [E rounded up to a multiple of 4, >= 4], erow [same]"
        self.col_g, self.erow_g = GuardedScratch(dev, slots * 4), GuardedScratch(dev, slots * 4)
        self.aux_g = GuardedScratch(dev, lib.pope_csr_aux_elems(e) * 4)  # exactly pope_csr_aux_elems(E) ints
        self.guards = (self.col_g, self.erow_g, self.aux_g)
        self.need = lib.pope_csr_scratch_bytes(n, e)
        self.reset()

    def reset(self):
        self.rowptr.fill_(I_SENTINEL)
        for g in self.guards:
            g.view.fill_(0xF9)                                        # int32 0xF9F9F9F9 < 0: no slot, row or flag
        self.before = [g.snapshot() for g in self.guards]

    def run(self, ptr, nbytes):
        args = (_p(self.ei), self.e, self.n, _p(self.rowptr), self.col_g.ptr, self.erow_g.ptr, self.aux_g.ptr, ptr, nbytes)
        rc = self.lib.pope_csr_build_canonical(*args, _stream()) if self.canonical else self.lib.pope_csr_build(*args, 0, _stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        i32 = lambda g: g.view.cpu().numpy().view(np.int32)[:self.e]
        return {"rowptr": self.rowptr.cpu().numpy(), "col": i32(self.col_g), "erow": i32(self.erow_g)}

    def check(self, out):
        for k, w in self.want.items():
            assert np.array_equal(out[k], w), (k, int((out[k] != w).sum()))

    def untouched(self):
        return bool((self.rowptr == I_SENTINEL).all()) and all(g.unchanged_since(b) for g, b in zip(self.guards, self.before))


def _csr(e, **kw):
    graph = {k: kw.pop(k) for k in ("hub",) if k in kw}
    return lambda dev, lib: CsrCall(dev, lib, *_csr_graph(e, **graph), **kw)


_row("pope_csr_build", "sorted-E256", _csr(256), 256, branch="sorted list, E even: edges in pairs; a full last chunk")
_row("pope_csr_build", "sorted-E255", _csr(255), 255, branch="sorted list, E odd: one edge at a time; one chunk")
_row("pope_csr_build", "sorted-E257", _csr(257), 257, branch="sorted list, E odd; a second chunk of one slot")
_row("pope_csr_build", "sorted-E1000-hub700", _csr(1000, hub=(3, 700)), 1000, branch="a row that spans several 256-slot chunks (aux)")
_row("pope_csr_build", "shuffled-E257", _csr(257, shuffled=True), 258, branch="the counting path: counts, cursors, scan and row-sort temporaries")
_row("pope_csr_build", "shuffled-E1000-hub700", _csr(1000, hub=(3, 700), shuffled=True), 1001, branch="the counting path with a spanning row")
_row("pope_csr_build_canonical", "shuffled-E256", _csr(256, canonical=True, shuffled=True), 256, branch="index check flag at offset 0, then the counting path")
_row("pope_csr_build_canonical", "sorted-E255", _csr(255, canonical=True), 255, branch="the counting path whatever the order")
_row("pope_csr_build_canonical", "shuffled-E1000-hub700", _csr(1000, hub=(3, 700), canonical=True, shuffled=True), 1000, branch="a spanning row")


# =====================================================================================================================================
# BFS: pope_geodesic_bfs, the _begin / _finish pair, pope_geodesic_run, pope_geodesic_column_stats (goldens, the CPU oracle)
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _bfs_graph(name, k):
    """(edge_index int64, n, anchors [k], hops int32 [n, k]) -- the golden's own anchors and hop counts where it has k of them, else
    anchors drawn with a fixed seed and the CPU oracle's hop counts, as test_geodesic_gpu.py's tests take them."""
    if name == "level_table":
        from graphpope_amd import synth
        ei, n = synth.rmat(12, edge_factor=5, seed=7)                 # test_geodesic_gpu.level_table_graph
        golden = None
    else:
        golden = load_golden(os.path.join(GOLDEN, "geodesic_%s.npz" % name))
        ei, n = golden["edge_index"].astype(np.int64), int(golden["num_nodes"])
    if golden is not None and len(golden["anchors"]) >= k:
        return ei, n, np.ascontiguousarray(golden["anchors"][:k], dtype=np.int64), np.ascontiguousarray(golden["hops"][:, :k])
    anchors = np.random.RandomState(k).choice(np.arange(n), k).astype(np.int64)
    return ei, n, anchors, _oracle().geodesic_hops(ei, n, anchors)


class BfsCall(Call):
    CAPACITY = 8

    def __init__(self, dev, lib, graph, k, split=False, live_mode=None):
        from graphpope_amd import _lib, engine
        self.lib, self.split, self.k = lib, split, k
        self.entry = "pope_geodesic_bfs_begin+finish" if split else "pope_geodesic_bfs"
        ei, self.n, self.anchors, self.want = _bfs_graph(graph, k)
        if live_mode is not None:                                     # the cell of the level-kernel table (tests/test_abi.py) the row is for
            from test_abi import level_kernel_wanted
            name = ctypes.create_string_buffer(64)
            _lib.check(lib.pope_level_kernel_name(self.n, k, name, 64))
            assert name.value.decode() == level_kernel_wanted(k, live_mode), name.value
        self.csr = engine.build_csr(_to(ei, dev), self.n)
        self.planes = torch.empty((self.CAPACITY + 1, self.n, lib.pope_words(k)), dtype=torch.int64, device=dev)
        self.need = lib.pope_bfs_scratch_bytes(self.n, self.csr.num_edges, k)
        self.max_hop, self.bits = ctypes.c_int32(0), ctypes.c_int32(0)
        self.reset()

    def reset(self):
        self.planes.fill_(-1)                                         # "planes need not be initialised"
        self.max_hop.value = self.bits.value = I_SENTINEL

    def run(self, ptr, nbytes):
        c, lib = self.csr, self.lib
        args = (_p(c.rowptr), _p(c.col), _p(c.erow), _p(c.aux), c.num_nodes, c.num_edges, ctypes.c_void_p(self.anchors.ctypes.data), self.k,
                _p(self.planes), self.CAPACITY, ptr, nbytes)
        tail = (ctypes.byref(self.max_hop), ctypes.byref(self.bits), _stream())
        if self.split:
            rc = lib.pope_geodesic_bfs_begin(*args, _stream())
            finish = lib.pope_geodesic_bfs_finish(*args, *tail)      # (after a refused _begin: refused for the same reason, nothing to wait for)
            assert rc == 0 or finish == rc, (rc, finish)
            rc = rc or finish
        else:
            rc = lib.pope_geodesic_bfs(*args, *tail)
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        from graphpope_amd import engine
        bits = self.bits.value
        out = {"max_hop": np.array([self.max_hop.value]), "n_hop_bits": np.array([bits])}
        if 0 <= bits <= self.CAPACITY:
            out["planes"] = self.planes[:1 + bits].cpu().numpy()
            out["hops"] = engine.hop_matrix(engine.HopPlanes(self.planes, bits, self.max_hop.value, self.n, self.k)).cpu().numpy()
        return out

    def check(self, out):
        assert np.array_equal(out["hops"], self.want), int((out["hops"] != self.want).sum())
        assert out["max_hop"][0] == max(int(self.want.max()), 0)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.planes == -1).all()) and self.max_hop.value == I_SENTINEL and self.bits.value == I_SENTINEL


for _split in (False, True):
    _entry = "pope_geodesic_bfs_begin+finish" if _split else "pope_geodesic_bfs"
    for _graph, _n in (("path201_odd", 201), ("rmat8_k130", 256)):
        for _k in (1, 64, 65):
            _row(_entry, "%s-K%d" % (_graph, _k), lambda dev, lib, g=_graph, k=_k, s=_split: BfsCall(dev, lib, g, k, s), _n * _k,
                 branch="W = %d%s" % (1 if _k <= 64 else 2, ", N odd, 200 levels" if _n == 201 else ""))
    for _mode in (1, 2, 3):
        _row(_entry, "level_table-K100-live%d" % _mode, lambda dev, lib, s=_split, m=_mode: BfsCall(dev, lib, "level_table", 100, s, m), 4096 * 100 + _mode,
             knobs=(("KNOB_LIVE_MODE", _mode, -1),), branch="live table: %s" % {1: "staged in LDS", 2: "read from global memory", 3: "behind its summary"}[_mode])


class GeodesicRunCall(Call):
    entry = "pope_geodesic_run"
    CAPACITY = 8

    def __init__(self, dev, lib, graph):
        self.lib = lib
        g = self.g = load_golden(os.path.join(GOLDEN, "geodesic_%s.npz" % graph))
        self.n, self.anchors = int(g["num_nodes"]), np.ascontiguousarray(g["anchors"], dtype=np.int64)
        self.k, self.f = len(self.anchors), g["x"].shape[1]
        assert self.k <= 256                                           # the merged prepare launch takes at most 256 anchors
        self.ei, self.x = _to(g["edge_index"].astype(np.int64), dev), _to(g["x"], dev)
        self.e = self.ei.shape[1]
        self.out = torch.empty((self.n, self.f + self.k), device=dev)
        self.need = lib.pope_geodesic_run_workspace_bytes(self.n, self.e, self.k, self.CAPACITY)
        self.max_hop, self.bits = ctypes.c_int32(0), ctypes.c_int32(0)
        self.ws = None
        self.reset()

    def reset(self):
        self.out.fill_(sb.SENTINEL)
        self.max_hop.value = self.bits.value = I_SENTINEL

    def run(self, ptr, nbytes):
        self.ws = ptr
        rc = self.lib.pope_geodesic_run(_p(self.ei), self.e, self.n, ctypes.c_void_p(self.anchors.ctypes.data), self.k, _p(self.x), self.f,
                                        _p(self.out), self.f + self.k, self.CAPACITY, ptr, nbytes, ctypes.byref(self.max_hop),
                                        ctypes.byref(self.bits), _stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        out = {"out": self.out.cpu().numpy(), "max_hop": np.array([self.max_hop.value]), "n_hop_bits": np.array([self.bits.value])}
        bits = self.bits.value
        if 0 <= bits <= self.CAPACITY and self.ws is not None:
            w = self.lib.pope_words(self.k)
            at = self.lib.pope_geodesic_run_planes(self.ws, self.n, self.e, self.k, self.CAPACITY)
            assert self.ws.value <= at and at + (self.CAPACITY + 1) * self.n * w * 8 <= self.ws.value + self.need
            hops = torch.empty((self.n, self.k), dtype=torch.int32, device=self.out.device)
            from graphpope_amd import _lib
            _lib.check(self.lib.pope_geodesic_hops(ctypes.c_void_p(at), bits, self.n, self.k, _p(hops), _stream()))
            out["hops"] = hops.cpu().numpy()
        return out

    def check(self, out):
        g, f = self.g, self.f
        assert np.array_equal(out["out"][:, :f], g["x"])
        assert np.array_equal(out["out"][:, f:].view(np.uint32), g["emb"].view(np.uint32))
        assert np.array_equal(out["hops"], g["hops"]) and out["max_hop"][0] == max(int(g["hops"].max()), 0)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.out == sb.SENTINEL).all()) and self.bits.value == I_SENTINEL


for _merge in (1, 0):                       # fill independence: test_geodesic_gpu.test_one_prepare_launch_gives_the_same_bits; here the bands
    _row("pope_geodesic_run", "rmat8_k130-merge%d" % _merge, lambda dev, lib: GeodesicRunCall(dev, lib, "rmat8_k130"), 130 + _merge,
         knobs=(("KNOB_PREPARE_MERGE", _merge, 1),), props=("contained", "refused"),
         branch="k_prepare: clear + seed + CSR in one launch" if _merge else "separate launches")
    _row("pope_geodesic_run", "path201_odd-merge%d" % _merge, lambda dev, lib: GeodesicRunCall(dev, lib, "path201_odd"), 6 + _merge,
         knobs=(("KNOB_PREPARE_MERGE", _merge, 1),), props=("contained", "refused"), branch="N * W odd, deeper than the speculative window")


class ColumnStatsCall(Call):
    entry = "pope_geodesic_column_stats"

    def __init__(self, dev, lib, k):
        from graphpope_amd import engine
        self.lib, self.k = lib, k
        ei, self.n, anchors, want = _bfs_graph("rmat8_k130", k)
        self.hp = engine.bfs(engine.build_csr(_to(ei, dev), self.n), anchors)
        hops = engine.hop_matrix(self.hp).cpu().numpy()             # the expected values: column sums and reach counts of the hop matrix
        assert np.array_equal(hops, want)
        self.want = {"hop_sum": np.where(hops >= 0, hops, 0).sum(axis=0).astype(np.int64), "reach": (hops >= 0).sum(axis=0).astype(np.int64)}
        self.hop_sum, self.reach = (torch.empty(k, dtype=torch.int64, device=dev) for _ in range(2))
        self.need = lib.pope_column_stats_scratch_bytes(k)
        self.reset()

    def reset(self):
        self.hop_sum.fill_(I_SENTINEL)
        self.reach.fill_(I_SENTINEL)

    def run(self, ptr, nbytes):
        hp = self.hp
        rc = self.lib.pope_geodesic_column_stats(_p(hp.planes), hp.n_hop_bits, self.n, self.k, _p(self.hop_sum), _p(self.reach), ptr, nbytes, _stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return {"hop_sum": self.hop_sum.cpu().numpy(), "reach": self.reach.cpu().numpy()}

    def check(self, out):
        assert np.array_equal(out["hop_sum"], self.want["hop_sum"]) and np.array_equal(out["reach"], self.want["reach"])

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.hop_sum == I_SENTINEL).all()) and bool((self.reach == I_SENTINEL).all())


for _k in (1, 65, 200):
    _row("pope_geodesic_column_stats", "rmat8-K%d" % _k, lambda dev, lib, k=_k: ColumnStatsCall(dev, lib, k), _k, branch="%d words per node" % ((_k + 63) // 64))


# =====================================================================================================================================
# Pairwise: pope_pairwise_features, _by_id, pope_pairwise_minmax (pairwise_plan_cases.CASES: the smallest row of each plan)
# =====================================================================================================================================
class PairwiseCall(Call):
    ATOL = 1e-5                                                        # test_pairwise_plan_gpu.py: the project's gate on the scaled values

    def __init__(self, dev, lib, row, fn):
        from graphpope_amd import _lib
        self.lib, self.row, self.fn = lib, row, fn
        n, d, k, f, has_x, by_id, knob = row
        self.entry = "pope_pairwise_features_by_id" if by_id else "pope_pairwise_features" if has_x else "pope_pairwise_minmax"
        buf = ctypes.create_string_buffer(256)
        _lib.check(lib.pope_pairwise_kernel_name(n, d, k, f, has_x, by_id, pw_cases.CUS, buf, 256))
        assert buf.value.decode() == pw_cases.CASES[row], buf.value
        emb, anchors = pw_cases.inputs(n, d, k)
        self.want = pw_cases.want64(n, d, k, fn)
        self.emb = _to(np.array(emb), dev)
        self.ids, self.rows = _to(np.array(anchors, dtype=np.int64), dev), _to(emb[anchors], dev)
        self.x_host = pc.features(n, f) if has_x else None
        self.x = _to(self.x_host, dev) if has_x else None
        self.out = torch.empty((n, f + k), device=dev)
        self.need = (lib.pope_pairwise_by_id_scratch_bytes if by_id else lib.pope_pairwise_scratch_bytes)(n, k, d)
        self.reset()

    def reset(self):
        self.out.fill_(sb.SENTINEL)

    def run(self, ptr, nbytes):
        from graphpope_amd import _lib
        n, d, k, f, has_x, by_id, _ = self.row
        metric, lib = _lib.METRIC[self.fn], self.lib
        if by_id:
            rc = lib.pope_pairwise_features_by_id(_p(self.x), f if has_x else 0, _p(self.emb), n, d, _p(self.ids), k, metric, _p(self.out), f + k, f,
                                                  ptr, nbytes, _stream())
        elif has_x:
            rc = lib.pope_pairwise_features(_p(self.x), f, _p(self.emb), n, d, _p(self.rows), k, metric, _p(self.out), f + k, f, ptr, nbytes, _stream())
        else:
            rc = lib.pope_pairwise_minmax(_p(self.emb), n, d, _p(self.rows), k, metric, _p(self.out), f + k, f, ptr, nbytes, _stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return {"out": self.out.cpu().numpy()}

    def check(self, out):
        f, got = self.row[3], out["out"]
        if self.x_host is not None:
            assert np.array_equal(got[:, :f].view(np.uint32), self.x_host.view(np.uint32))
        else:
            assert (got[:, :f] == sb.SENTINEL).all()                  # no x: the embedding columns alone are written
        emb = got[:, f:]
        assert np.isfinite(emb).all() and float(np.abs(emb - self.want).max()) <= self.ATOL, float(np.abs(emb - self.want).max())
        if self.fn == "euclidean":
            assert emb[5, 0] == 0.0 and emb[7, 0] == 0.0

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.out == sb.SENTINEL).all())


# (row of pairwise_plan_cases.CASES, metric, pipeline): the smallest row of each plan per entry point, under each knob value the table uses
_PAIRWISE = [
    ((257, 128, 256, 8, 1, 0, 0), "euclidean", "persistent, one set beside the side copy"),
    ((257, 128, 256, 8, 1, 0, 2), "distance", "persistent, knob 2"),
    ((257, 128, 256, 8, 1, 0, 1), "similarity", "one tile per block, vectors, carries the copy (knob 1)"),
    ((257, 130, 256, 8, 1, 0, 0), "euclidean", "one tile per block, generic operands"),
    ((257, 128, 256, 6, 1, 0, 0), "distance", "pope_concat in front of the persistent kernel"),
    ((33, 4, 5, 0, 0, 1, 0), "euclidean", "by id, persistent, two sets"),
    ((257, 128, 256, 8, 1, 1, 0), "similarity", "by id, persistent beside the side copy"),
    ((257, 128, 256, 8, 1, 1, 3), "distance", "by id, persistent, knob 3"),
    ((257, 128, 257, 0, 0, 1, 1), "euclidean", "by id, one tile per block: the anchor rows gathered into the scratch (knob 1)"),
    ((257, 7, 256, 8, 1, 1, 0), "similarity", "by id, gathered anchor rows, generic operands, carries the copy"),
    ((257, 36, 257, 0, 0, 0, 0), "euclidean", "minmax, persistent, two sets, zero-padded depth"),
    ((257, 128, 256, 0, 0, 0, 2), "similarity", "minmax, persistent, knob 2"),
    ((257, 128, 256, 0, 0, 0, 3), "distance", "minmax, persistent, knob 3"),
    ((257, 7, 257, 0, 0, 0, 0), "distance", "minmax, one tile per block, generic operands"),
    ((257, 132, 255, 0, 0, 0, 0), "euclidean", "minmax, one tile per block, vectors"),
]
for _r, _fn, _branch in _PAIRWISE:
    assert _r in pw_cases.CASES and _r[0] <= pw_cases.GPU_MAX_N
    _entry = "pope_pairwise_features_by_id" if _r[5] else "pope_pairwise_features" if _r[4] else "pope_pairwise_minmax"
    _row(_entry, "n%d_d%d_k%d_f%d_x%d_id%d_knob%d-%s" % (_r + (_fn,)), lambda dev, lib, r=_r, fn=_fn: PairwiseCall(dev, lib, r, fn),
         _r[0] * _r[2] * 1000 + _r[1], knobs=(("KNOB_PAIRWISE_KERNEL", _r[6], 0),), branch=_branch)


# =====================================================================================================================================
# pope_betweenness_batch (the star with pendant paths of test_anchor_select_gpu.py; test_betweenness_cpu.replay = NetworkX's additions)
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _star():
    import test_anchor_select_gpu as tas
    import test_betweenness_cpu as tbc
    ei, n = tas._star_with_pendant_paths()
    return ei, n, tbc.replay(ei, n, normalized=False)


class BetweennessCall(Call):
    entry = "pope_betweenness_batch"

    def __init__(self, dev, lib, batch):
        from graphpope_amd import engine
        self.lib = lib
        ei, self.n, self.want = _star()
        assert self.n == 199
        self.batch = self.n if batch == "N" else batch
        eid = _to(ei, dev)
        self.by_source, self.by_target = engine.insertion_csr(eid, self.n), engine.insertion_csr(eid.flip(0).contiguous(), self.n)
        self.bc = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.need = lib.pope_betweenness_scratch_bytes(self.n, self.batch)
        self.start = 0.0
        self.reset()

    def reset(self):
        self.bc.fill_(self.start)                                     # "the caller zeroes bc"

    def run(self, ptr, nbytes):
        (rp_s, col_s, e_s), (rp_t, col_t, e_t) = self.by_source, self.by_target
        rc = 0
        for lo in range(0, self.n, self.batch):                       # the batches in source order on one stream, one scratch
            rc = self.lib.pope_betweenness_batch(_p(rp_s), _p(col_s), e_s, _p(rp_t), _p(col_t), e_t, self.n, lo, min(self.batch, self.n - lo), _p(self.bc),
                                                 None, None, None, None, ptr, nbytes, _stream())
            if rc:
                break
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return {"bc": self.bc.cpu().numpy()}

    def check(self, out):
        assert np.array_equal(out["bc"].view(np.uint64), self.want.view(np.uint64)), int((out["bc"].view(np.uint64) != self.want.view(np.uint64)).sum())

    def untouched(self):
        return bool((self.bc == self.start).all())


for _b in (1, 7, "N"):
    _row("pope_betweenness_batch", "star199-batch%s" % _b, lambda dev, lib, b=_b: BetweennessCall(dev, lib, b), 199 if _b == "N" else _b,
         branch="%s source(s) per call: 36 bytes per (source, node)" % _b)


# =====================================================================================================================================
# pope_n2v_accumulate_det (node2vec_det_cases: the ordered-sum case and its contract restated)
# =====================================================================================================================================
class AccumulateCall(Call):
    entry = "pope_n2v_accumulate_det"
    D = 32

    def __init__(self, dev, lib, m):
        self.lib, self.m = lib, m
        ids, contrib, self.prior = n2v_cases.ordered_sum_case(self.D)
        self.want, self.want_touched = n2v_cases.accumulate_reference(ids[:m], contrib[:m], self.prior)
        self.ids, self.contrib = _to(ids[:m], dev), _to(contrib[:m], dev)
        self.grad, self.touched = _to(self.prior, dev), torch.zeros(n2v_cases.N, dtype=torch.uint8, device=dev)
        self.need = lib.pope_n2v_accumulate_det_scratch_bytes(m, n2v_cases.N)
        assert self.need == 4 * (n2v_cases.N + 1) + 8 * m

    def reset(self):
        self.grad.copy_(torch.from_numpy(self.prior))
        self.touched.zero_()

    def run(self, ptr, nbytes):
        rc = self.lib.pope_n2v_accumulate_det(_p(self.ids), self.m, _p(self.contrib), self.D, n2v_cases.N, _p(self.grad), _p(self.touched), None, 0, 1.0,
                                              None, ptr, nbytes, _stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return {"grad": self.grad.cpu().numpy(), "touched": self.touched.cpu().numpy()}

    def check(self, out):
        assert np.array_equal(out["touched"], self.want_touched)
        assert np.array_equal(out["grad"].view(np.int32), self.want.view(np.int32)), int((out["grad"].view(np.int32) != self.want.view(np.int32)).sum())

    def untouched(self):
        return np.array_equal(self.grad.cpu().numpy().view(np.int32), self.prior.view(np.int32)) and not bool(self.touched.any())


for _m in (n2v_cases.M, 200, 1):
    _row("pope_n2v_accumulate_det", "M%d-N%d" % (_m, n2v_cases.N), lambda dev, lib, m=_m: AccumulateCall(dev, lib, m), _m,
         branch="lists of 1 500, 65, 64 and 1 entries" if _m == n2v_cases.M else "a prefix of the same entries")


# =====================================================================================================================================
# pope_logreg_loss_grad (logreg_cases: objective cases, the longdouble restatement and its bounds)
# =====================================================================================================================================
class LogregCall(Call):
    entry = "pope_logreg_loss_grad"
    refusal = ERR_INVALID

    def __init__(self, dev, lib, case):
        self.lib, self.case = lib, case
        table, sel, _, y, w, self.l2 = logreg_cases.objective_inputs(case)
        assert sel is None
        self.z, self.y, self.w = _to(np.array(table), dev), _to(y.astype(np.int32), dev), _to(np.array(w), dev)
        self.ldz = table.shape[1]
        self.out = torch.empty(1 + w.size, dtype=torch.float64, device=dev)
        self.need = lib.pope_logreg_scratch_bytes(case["m"], case["d"], case["classes"])
        self.reset()

    def reset(self):
        self.out.fill_(7.0)

    def run(self, ptr, nbytes):
        c = self.case
        rc = self.lib.pope_logreg_loss_grad(_p(self.z), self.ldz, self.z.shape[0], None, c["m"], c["d"], _p(self.y), c["classes"], int(c["icpt"]),
                                            _p(self.w), self.l2, _p(self.out), ctypes.c_void_p(self.out.data_ptr() + 8), ptr, nbytes, _stream())
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return {"loss_grad": self.out.cpu().numpy()}

    def check(self, out):
        ref, lb, gb = logreg_cases.reference(self.case)
        loss, grad = out["loss_grad"][0], out["loss_grad"][1:]
        el = abs(float(np.longdouble(loss) - ref["loss"]))
        eg = np.abs((grad.astype(np.longdouble) - ref["grad"]).astype(np.float64))
        assert el <= lb and (eg <= gb).all(), (el / lb, float((eg / gb).max()))

    def untouched(self):
        return bool((self.out == 7.0).all())


def _logreg_rows():
    """The smallest binary and the smallest multiclass objective case on each side of pope_logreg_slice_rows() = 256 rows."""
    table = [c for c in logreg_cases.objective_cases() if not c["nan"] and not c["ids"] and c["w"] != "zero"]
    out = []
    for classes in (2, 3):
        mine = [c for c in table if c["classes"] == classes]
        for side in (lambda m: m <= logreg_cases.SLICE_DEFAULT, lambda m: m > logreg_cases.SLICE_DEFAULT):
            out.append(min((c for c in mine if side(c["m"])), key=lambda c: (c["m"], c["d"], c["pad"])))
    return out


for _case in _logreg_rows():
    _row("pope_logreg_loss_grad", _case["id"], lambda dev, lib, c=_case: LogregCall(dev, lib, c), _case["m"] * _case["d"],
         branch="%s, %s slice" % ("binomial" if _case["classes"] == 2 else "multinomial", "one" if _case["m"] <= logreg_cases.SLICE_DEFAULT else "a second"))

assert len({r.id for r in ROWS}) == len(ROWS)
