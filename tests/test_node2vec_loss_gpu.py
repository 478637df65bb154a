"""The node2vec loss kernels, the scan of the deterministic sum and SparseAdam on the device, against tests/node2vec_loss_cases.py:
pope_n2v_loss_grad (atomic form) and pope_n2v_position_grads + pope_n2v_accumulate_det (deterministic pair) within error bounds derived
from their arithmetic, element by element, against a float64 restatement -- at the reference's walk shape (len 21, C 10, D 128), at
every width and slab, at the trip counts of the pair and id loops, at the rows-per-wave edge and at the largest LDS request each entry
point accepts; pope_n2v_accumulate_det bit for bit where the scan crosses a wave and a round of 8192 nodes; pope_n2v_sparse_adam bit
for bit against the documented float32 update.  Every test prints its largest error / bound before it asserts."""
import numpy as np
import pytest
import torch

import node2vec_loss_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


@pytest.fixture(autouse=True)
def mode_off():
    from graphpope_amd import sage
    assert not sage.is_deterministic(), "an earlier test left the switch on"
    yield
    sage.set_deterministic(False)


_tables = {}


def _table(dev, n, d):
    if (n, d) not in _tables:
        _tables[n, d] = torch.from_numpy(cases.table(n, d).copy()).to(dev)
    return _tables[n, d]


def _ratio(err, bound):
    """The largest err / bound; an error where the bound is 0 counts as infinite."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


def _check_grad(got, touched, res, bound, n, what):
    """Every element of the occurring rows within its bound; touched exactly those rows; every other row bit-zero."""
    occurs = np.zeros(n, dtype=bool)
    occurs[res.nodes] = True
    ratio = _ratio(np.abs(got[res.nodes].astype(np.float64) - res.grad), bound)
    assert np.array_equal(touched.astype(bool), occurs), what
    assert not got[~occurs].view(np.int32).any(), what
    return ratio


# ---- 1. the atomic form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.ATOMIC_CASES, ids=lambda c: c.name)
def test_atomic_form_within_derived_bounds(dev, case):
    from graphpope_amd import node2vec
    worst = {"grad": 0.0, "loss": 0.0}
    failures = []
    for n in cases.POPULATIONS:
        for negative in cases.NEGATIVE:
            emb, rows, scale, res, b = cases.solved(case, n, negative)
            emb_t, rows_t = _table(dev, n, case.d), torch.from_numpy(rows.copy()).to(dev)
            acc = torch.zeros(1, dtype=torch.float64, device=dev)
            grad = torch.zeros(n, case.d, device=dev)
            touched = torch.zeros(n, dtype=torch.uint8, device=dev)
            node2vec.loss_grad(emb_t, rows_t, case.c, bool(negative), scale, acc, grad, touched)
            what = f"{case.name} N {n} negative {negative}"
            g = _check_grad(grad.cpu().numpy(), touched.cpu().numpy(), res, b["grad_atomic"], n, what)
            l1 = abs(float(acc) - res.loss) / b["loss"]
            only = torch.zeros(1, dtype=torch.float64, device=dev)
            node2vec.loss_grad(emb_t, rows_t, case.c, bool(negative), scale, only)           # grad = None: the loss alone
            l2 = abs(float(only) - res.loss) / b["loss"]
            print(f"{what}: atomic grad error/bound {g:.3f} loss error/bound {l1:.3f} loss-only {l2:.3f}")
            worst["grad"], worst["loss"] = max(worst["grad"], g), max(worst["loss"], l1, l2)
            if not (g <= 1.0 and l1 <= 1.0 and l2 <= 1.0):
                failures.append((what, g, l1, l2))
    print(f"FAMILY {case.family} atomic: grad {worst['grad']:.3f} loss {worst['loss']:.3f}")
    assert not failures, failures


# ---- 2. the deterministic pair ---------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", cases.DET_CASES, ids=lambda c: c.name)
def test_deterministic_pair_within_derived_bounds(dev, case):
    from graphpope_amd import node2vec
    worst = {"contrib": 0.0, "grad": 0.0, "loss": 0.0}
    failures = []
    lo, hi = (2, min(5, case.r)) if case.r >= 3 else (case.r - 1, case.r)    # the sub-batch: rows [2:5], or what the case has of them
    for n in cases.POPULATIONS:
        for negative in cases.NEGATIVE:
            emb, rows, scale, res, b = cases.solved(case, n, negative)
            emb_t, rows_t = _table(dev, n, case.d), torch.from_numpy(rows.copy()).to(dev)
            what = f"{case.name} N {n} negative {negative}"
            valid = torch.from_numpy(res.valid).to(dev)
            ids, contrib, row_loss = node2vec.position_grads(emb_t, rows_t, case.c, bool(negative), scale)
            want_ids = np.where(res.valid[:, None], rows, -1).astype(np.int32).reshape(-1)
            assert ids.dtype == torch.int32 and np.array_equal(ids.cpu().numpy(), want_ids), what     # exact; a bad row: all -1
            per_row = contrib.view(case.r, case.length, case.d)
            got = per_row.cpu().numpy().astype(np.float64)
            c_ratio = _ratio(np.abs(got - res.pos_grad)[res.valid], b["contrib"][res.valid])
            got_loss = row_loss.cpu().numpy()
            assert not got_loss[~res.valid].any(), what                                              # a bad row: loss 0
            r_ratio = _ratio(np.abs(got_loss - res.row_loss)[res.valid], b["row_loss"][res.valid])
            # two calls: the same bits; a call on a slice of the rows: the bits of that slice
            again = node2vec.position_grads(emb_t, rows_t, case.c, bool(negative), scale)
            assert torch.equal(again[0], ids) and torch.equal(again[2].view(torch.int64), row_loss.view(torch.int64)), what
            assert torch.equal(_bits(again[1].view(case.r, -1)[valid]), _bits(per_row.reshape(case.r, -1)[valid])), what
            part = node2vec.position_grads(emb_t, rows_t[lo:hi].contiguous(), case.c, bool(negative), scale)
            assert torch.equal(part[0], ids.view(case.r, -1)[lo:hi].reshape(-1)), what
            assert torch.equal(part[2].view(torch.int64), row_loss[lo:hi].view(torch.int64)), what
            assert torch.equal(_bits(part[1].view(hi - lo, -1)[valid[lo:hi]]), _bits(per_row.reshape(case.r, -1)[lo:hi][valid[lo:hi]])), what
            # the ordered sum of the stored rows
            acc = torch.zeros(1, dtype=torch.float64, device=dev)
            grad = torch.zeros(n, case.d, device=dev)
            touched = torch.zeros(n, dtype=torch.uint8, device=dev)
            node2vec.accumulate_det(ids, contrib, grad, touched, row_loss, scale, acc)
            g_ratio = _check_grad(grad.cpu().numpy(), touched.cpu().numpy(), res, b["grad_det"], n, what)
            l_ratio = abs(float(acc) - res.loss) / b["loss"]
            print(f"{what}: contrib error/bound {c_ratio:.3f} row_loss {r_ratio:.3f} det grad {g_ratio:.3f} loss {l_ratio:.3f}")
            worst["contrib"], worst["grad"] = max(worst["contrib"], c_ratio), max(worst["grad"], g_ratio)
            worst["loss"] = max(worst["loss"], r_ratio, l_ratio)
            if not (c_ratio <= 1.0 and r_ratio <= 1.0 and g_ratio <= 1.0 and l_ratio <= 1.0):
                failures.append((what, c_ratio, r_ratio, g_ratio, l_ratio))
    print(f"FAMILY {case.family} deterministic: contrib {worst['contrib']:.3f} grad {worst['grad']:.3f} loss {worst['loss']:.3f}")
    assert not failures, failures


# ---- 3. the scan of the ordered sum ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.SCAN_N)
def test_ordered_sum_where_the_scan_crosses_waves_and_rounds(dev, n):
    from graphpope_amd import node2vec
    ids, contrib, prior, want, want_touched = cases.scan_case(n)
    grad = torch.from_numpy(prior.copy()).to(dev)
    touched = torch.zeros(n, dtype=torch.uint8, device=dev)
    node2vec.accumulate_det(torch.from_numpy(ids.copy()).to(dev), torch.from_numpy(contrib.copy()).to(dev), grad, touched, None, 1.0, None)
    got = grad.cpu().numpy()
    assert np.array_equal(touched.cpu().numpy(), want_touched)                                     # exactly the nodes with a valid entry
    wrong = np.nonzero((got.view(np.int32) != want.view(np.int32)).any(axis=1))[0]
    assert wrong.size == 0, (n, wrong[:10].tolist(), wrong.size)


# ---- 4. SparseAdam, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", cases.ADAM_SHAPES)
def test_sparse_adam_is_the_documented_update_bit_for_bit(dev, n, d):
    from graphpope_amd import node2vec
    rng = np.random.default_rng(n + d)
    p = rng.standard_normal((n, d)).astype(np.float32)
    m, v = np.zeros_like(p), np.zeros_like(p)
    emb, m1, m2 = torch.from_numpy(p.copy()).to(dev), torch.zeros(n, d, device=dev), torch.zeros(n, d, device=dev)
    grad, touched = torch.zeros(n, d, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    failures = []
    for step, (rows, vals) in enumerate(cases.sparse_adam_steps(n, d), start=1):
        g = np.zeros_like(p)
        g[rows] = vals
        grad.copy_(torch.from_numpy(g))
        touched[torch.from_numpy(rows).to(dev)] = 1
        before = p
        on_device = [t.cpu().numpy() for t in (emb, m1, m2)]                                      # what the call finds
        p, m, v = cases.sparse_adam_reference(p, m, v, g, rows, cases.ADAM_LR, *cases.ADAM_BETAS, cases.ADAM_EPS, step)
        node2vec.sparse_adam(emb, grad, touched, m1, m2, cases.ADAM_LR, *cases.ADAM_BETAS, cases.ADAM_EPS, step)
        assert not grad.any() and not touched.any(), step                                         # gradient rows and flags: cleared
        idle = np.ones(n, dtype=bool)
        idle[rows] = False
        for name, now, want, was in zip(("emb", "exp_avg", "exp_avg_sq"), (emb, m1, m2), (p, m, v), on_device):
            got = now.cpu().numpy()
            assert np.array_equal(got[idle].view(np.int32), was[idle].view(np.int32)), (name, step)   # unflagged rows: bit-unchanged
            differ = int((got.view(np.int32) != want.view(np.int32)).sum())
            print(f"N {n} D {d} step {step} {name}: {differ} of {len(rows) * d} updated elements differ from the restatement")
            if differ:
                failures.append((name, step, differ))
        if len(rows):
            assert not np.array_equal(p[rows], before[rows])
    assert not failures, failures
