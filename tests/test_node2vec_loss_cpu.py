"""tests/node2vec_loss_cases.py without a GPU: the float64 restatement of pope_n2v_loss_grad equals torch float64 autograd of PyG's loss
on the window matrices; every case keeps the invariants its bounds rest on (P, the LDS formulas of include/graphpope_hip.h, |out| < 6,
T < 8000) and every derived gradient bound stays below 1e-4 of the magnitude it is relative to; the two entry points refuse the first
row length past their LDS limit before any HIP call; and the float32 restatement of SparseAdam is torch.optim.SparseAdam's arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

import node2vec_loss_cases as cases
from test_node2vec_gpu import _pyg_loss, _windows


# ---- the restatement against autograd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [cases.CASES[0], cases.CASES[2], next(c for c in cases.CASES if c.family == "width" and c.d == 96)],
                         ids=lambda c: c.name)
def test_restatement_equals_float64_autograd_of_pygs_loss(case):
    """Positive rows from population 40, negative rows from population 40 too (other rows: the case of the negative call), one table."""
    n = 40
    emb, pos, scale, res_pos, _ = cases.solved(case, n, 0)
    neg = np.ascontiguousarray(pos[::-1, ::-1])                                # other rows over the same table
    res_neg = cases.reference(emb, neg, case.c, 1, scale)
    w = torch.from_numpy(emb.astype(np.float64)).requires_grad_(True)
    loss = _pyg_loss(w, _windows(torch.from_numpy(pos.copy()), case.c), _windows(torch.from_numpy(neg), case.c))
    loss.backward()
    want_loss, want_grad = float(loss.detach()), w.grad.numpy()
    got_loss = res_pos.loss + res_neg.loss
    got, mag = np.zeros((n, case.d)), np.zeros((n, case.d))
    for res in (res_pos, res_neg):
        got[res.nodes] += res.grad
        mag[res.nodes] += res.grad_mag
    assert abs(got_loss - want_loss) <= 1e-12 * abs(want_loss), (got_loss, want_loss)
    assert np.isfinite(got).all() and (mag[np.unique(pos)] > 0).all()
    assert (np.abs(got - want_grad) <= 1e-12 * mag).all(), float((np.abs(got - want_grad) / np.maximum(mag, 1e-300)).max())
    # the pieces are consistent: a position's rows add up to the node's row, the rows' losses to the call's
    for res, rows in ((res_pos, pos), (res_neg, neg)):
        assert res.valid.all() and res.terms == case.r * case.pairs and int(res.n_v.sum()) == rows.size
        assert np.array_equal(res.nodes, np.unique(rows))
        assert abs(res.loss - scale * res.row_loss.sum()) <= 1e-15 * abs(res.loss)
        v = int(res.nodes[0])
        at = rows == v
        assert res.n_v[0] == at.sum() and np.allclose(res.grad[0], res.pos_grad[at].sum(axis=0), rtol=0, atol=1e-15 * res.grad_mag[0].max())


# ---- the invariants of every case -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_case_invariants_and_bound_sizes(case):
    assert case.pairs == (case.length + 1 - case.c) * (case.c - 1) and 2 <= case.c <= case.length and case.d % 32 == 0 and 32 <= case.d <= 256
    if case.forms in ("both", "atomic"):
        assert cases.loss_grad_lds_bytes(case.length, case.c, case.d) <= cases.LDS_LIMIT
    if case.forms in ("both", "det"):
        assert cases.position_grads_lds_bytes(case.length, case.c, case.d) <= cases.LDS_LIMIT
    if case.forms == "det":
        assert cases.loss_grad_lds_bytes(case.length, case.c, case.d) > cases.LDS_LIMIT
    for n in cases.POPULATIONS:
        rows = cases.walk_rows(case, n)
        assert rows.shape == (case.r, case.length)
        valid_ids = rows[(rows >= 0) & (rows < n)]
        if n == 5000:
            assert len(np.unique(valid_ids)) == len(valid_ids)                 # all distinct: nothing merges
        first_wave = np.unique(rows[:cases.ROWS_PER_WAVE])
        if n == 40 and case.r * case.length >= 64:
            assert len(first_wave) > cases.SLOTS and len(first_wave) < min(case.r, cases.ROWS_PER_WAVE) * case.length   # slots run out, ids repeat
        for negative in cases.NEGATIVE:
            emb, _, scale, res, b = cases.solved(case, n, negative)
            assert emb.dtype == np.float32 and emb.shape == (n, case.d) and scale == 1.0 / (case.r * case.pairs)
            assert res.max_out < cases.OUT_LIMIT, res.max_out
            bad_rows = 2 if case.bad else 0
            assert int(res.valid.sum()) == case.r - bad_rows and res.terms == (case.r - bad_rows) * case.pairs < cases.MAX_TERMS
            if case.bad:
                assert not res.valid[3] and not res.valid[5] and not res.pos_grad[[3, 5]].any() and not res.row_loss[[3, 5]].any()
            assert np.isfinite(res.grad).all() and (res.A[res.valid] > 0).all() and (res.grad_mag > 0).all()
            assert (np.abs(res.pos_grad) <= res.A * (1 + 1e-12)).all() and (np.abs(res.grad) <= res.grad_mag * (1 + 1e-12)).all()
            # every derived bound: below 1e-4 of the magnitude it is relative to
            assert (b["contrib"][res.valid] < 1e-4 * res.A[res.valid]).all()
            assert (b["grad_atomic"] < 1e-4 * res.grad_mag).all() and (b["grad_det"] < 1e-4 * res.grad_mag).all()
            assert 0 < b["loss"] < 1e-12 * res.scale * res.row_abs.sum()
            if n == 3:
                assert res.n_v.max() >= case.r * case.length // 4               # long chains on few nodes


def test_largest_lds_lengths_come_from_the_headers_formulas():
    assert cases.loss_grad_lds_bytes(47, 2, 256) == 65136 <= cases.LDS_LIMIT < cases.loss_grad_lds_bytes(48, 2, 256)
    assert cases.position_grads_lds_bytes(63, 2, 256) <= cases.LDS_LIMIT < cases.position_grads_lds_bytes(64, 2, 256)
    assert (cases.LDS_LEN_LOSS_GRAD, cases.LDS_LEN_POSITION_GRADS) == (47, 63)
    assert {(c.length, c.forms) for c in cases.CASES if c.family == "largest-lds"} == {(47, "atomic"), (63, "det")}


def test_entry_points_refuse_the_first_length_past_the_lds_limit():
    """Before any HIP call.  At the largest accepted length the same null-pointer call gets past the LDS check."""
    from graphpope_amd import _lib
    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)              # `one`: non-null, never dereferenced -- every call fails validation
    for length, want in ((48, b"LDS"), (47, b"null pointer")):
        assert lib.pope_n2v_loss_grad(null if length == 47 else one, 10, 256, one, 2, length, 2, 0, 1.0, one, one, one, null) == _lib.ERR_INVALID
        msg = lib.pope_last_error()
        assert b"pope_n2v_loss_grad" in msg and want in msg, msg
    for length, want in ((64, b"LDS"), (63, b"null pointer")):
        assert lib.pope_n2v_position_grads(null if length == 63 else one, 10, 256, one, 2, length, 2, 0, 1.0, one, one, one,
                                           null) == _lib.ERR_INVALID
        msg = lib.pope_last_error()
        assert b"pope_n2v_position_grads" in msg and want in msg, msg


# ---- the scan case ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.SCAN_N)
def test_scan_case_reaches_the_edges_of_the_scan(n):
    ids, contrib, prior, want, touched = cases.scan_case(n)
    count = np.bincount(ids[(ids >= 0) & (ids < n)], minlength=n)
    for v in cases.SCAN_EDGES + (n - 1,):
        assert v >= n or count[v] == 3
    assert count.max() == cases.SCAN_LONG > 64 and (n <= 9000 or count[9000] == cases.SCAN_LONG)
    assert (ids == -1).sum() == 10 and (ids == n).sum() == 10 and len(ids) == cases.SCAN_M
    assert np.array_equal(touched, (count > 0).astype(np.uint8))
    idle = count == 0
    assert np.array_equal(want[idle].view(np.int32), prior[idle].view(np.int32)) and not np.array_equal(want[~idle], prior[~idle])
    # the values show the order: the same lists summed in descending entry order end in other bits
    other, _ = cases.det_cases.accumulate_reference(ids, contrib, prior, order=range(len(ids) - 1, -1, -1))
    assert not np.array_equal(other.view(np.int32), want.view(np.int32))


# ---- SparseAdam ------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """|a - b| in units of the last place of float32 (finite values of one sign or around zero: the ordered-integer distance)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def test_sparse_adam_restatement_is_torchs_arithmetic():
    """4 steps of torch.optim.SparseAdam (float32, CPU) at 130 x 96: the moments bit for bit, the parameters within one ulp -- torch's
    CPU kernel forms p + (-step_size * m / denom) through its sparse add, which does not always round as the plain sum does."""
    n, d = 130, 96
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal((n, d)).astype(np.float32)
    pt = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.SparseAdam([pt], lr=cases.ADAM_LR, betas=cases.ADAM_BETAS, eps=cases.ADAM_EPS)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    differing = []
    for step in range(1, 5):
        rows = np.nonzero(rng.random(n) < 0.4)[0]
        vals = (rng.standard_normal((len(rows), d)) * 10.0 ** rng.uniform(-3, 3, size=(len(rows), 1))).astype(np.float32)
        pt.grad = torch.sparse_coo_tensor(torch.from_numpy(rows)[None], torch.from_numpy(vals), (n, d))
        opt.step()
        g = np.zeros_like(p0)
        g[rows] = vals
        before = p.copy()
        p, m, v = cases.sparse_adam_reference(p, m, v, g, rows, cases.ADAM_LR, *cases.ADAM_BETAS, cases.ADAM_EPS, step)
        state = opt.state[pt]
        assert np.array_equal(m.view(np.int32), state["exp_avg"].numpy().view(np.int32)), step
        assert np.array_equal(v.view(np.int32), state["exp_avg_sq"].numpy().view(np.int32)), step
        dist = _ulps(p, pt.detach().numpy())
        differing.append(int((dist > 0).sum()))
        assert dist.max() <= 1, (step, int(dist.max()))
        idle = np.ones(n, dtype=bool)
        idle[rows] = False
        assert np.array_equal(p[idle].view(np.int32), before[idle].view(np.int32)) and not np.array_equal(p[rows], before[rows])
    print(f"parameter elements that differ from torch's CPU kernel, per step, of {n * d}: {differing}")


@pytest.mark.parametrize("n,d", cases.ADAM_SHAPES)
def test_sparse_adam_steps_cover_what_they_claim(n, d):
    steps = cases.sparse_adam_steps(n, d)
    assert len(steps) == 3 and len(steps[2][0]) == 0
    for rows, vals in steps[:2]:
        assert {v for v in (0, 63, 64, n - 1) if v < n} <= set(rows.tolist()) and vals.shape == (len(rows), d) and vals.dtype == np.float32
        assert len(np.unique(rows)) == len(rows) and (n < 10 or len(rows) < n)
        big = np.abs(vals).max(axis=1)
        assert big.min() < 1e-2 and (len(rows) < 2 or big.max() > 1e2)
