"""Logistic regression without a GPU: the restatement and the bounds of tests/logreg_cases.py hold themselves (row order, longdouble),
the restatement under scipy IS scikit-learn's lbfgs fit, the C ABI checks its arguments before any HIP call, and ``Node2Vec.test``
and the generator's parser refuse or default what they should before a GPU is needed."""
import ctypes

import numpy as np
import pytest

import logreg_cases as cases


def test_cases_cover_the_listed_extents():
    table = cases.objective_cases()
    assert len({c["id"] for c in table}) == len(table)
    assert {c["m"] for c in table} >= {1, 63, 64, 65, 257, cases.ragged_rows(cases.SLICE_DEFAULT)}
    assert cases.ragged_rows(256) > 2 * 256 and cases.ragged_rows(256) % 256 != 0
    assert {c["d"] for c in table if c["pad"]} >= {1, 3, 33, 128, 130}
    assert {c["classes"] for c in table} >= {2, 3, 7, 64} and {c["icpt"] for c in table} == {True, False}
    assert {c["w"] for c in table} == set(cases.W_MODES)
    assert sum(bool(c["ids"]) for c in table) >= 4 and sum(c["nan"] for c in table) == 2
    for n, d, C, *_ in cases.FIT_CASES:
        assert any((c["m"], c["d"], c["classes"]) == (n // 2, d, C) for c in table)
    for c in table:
        if c["ids"]:
            _, sel, *_ = cases.objective_inputs(c)
            assert sel[1] == sel[0] and (np.diff(sel[:50]) <= 0).all() and sel.min() >= 0 and sel.max() < c["ids"]
        if c["w"] == "big" and not c["nan"]:
            raw = np.asarray(cases.reference(c)[0]["raw"], dtype=np.float64)
            assert abs(np.abs(raw).max() - cases.BIG_RAW) < 1e-6 and (c["m"] < 60 or (raw.max() > 700 or raw.min() < -700))
    big2 = [c for c in table if c["w"] == "big" and c["classes"] == 2 and c["m"] >= 257]
    assert any(np.asarray(cases.reference(c)[0]["raw"], dtype=np.float64).max() > 710 for c in big2)       # exp(raw) would overflow ...
    assert any(np.asarray(cases.reference(c)[0]["raw"], dtype=np.float64).min() < -710 for c in big2)      # ... and so would exp(-raw)


def test_restatement_in_reversed_row_order_stays_inside_the_bounds():
    """float64, rows reversed (another summation order) against the longdouble evaluation: within the derived bounds, and the
    gradient bound is below 1e-10 max|grad| on every case -- tight enough that float32 accumulation cannot meet it."""
    worst_l = worst_g = worst_rel = 0.0
    for c in cases.objective_cases():
        if c["nan"]:
            continue
        _, _, z, y, w, l2 = cases.objective_inputs(c)
        ref, lb, gb = cases.reference(c)
        got = cases.restate(z, y, w, c["classes"], c["icpt"], l2, order=np.arange(c["m"])[::-1])
        el = abs(float(got["loss"] - ref["loss"]))
        eg = np.abs((got["grad"] - ref["grad"]).astype(np.float64))
        rel = gb.max() / float(np.abs(ref["grad"]).max())
        worst_l, worst_g, worst_rel = max(worst_l, el / lb), max(worst_g, float((eg / gb).max())), max(worst_rel, rel)
        assert np.isfinite(lb) and np.isfinite(gb).all() and (gb > 0).all()
        assert el <= lb and (eg <= gb).all(), c["id"]
        assert rel < 1e-10, (c["id"], rel)
    print(f"restatement, rows reversed: largest loss error / bound {worst_l:.3g}, gradient {worst_g:.3g}; "
          f"largest gradient bound / max|grad| {worst_rel:.3g}")


def test_restatement_keeps_a_nan_row():
    for c in cases.objective_cases():
        if c["nan"]:
            _, _, z, y, w, l2 = cases.objective_inputs(c)
            assert np.isnan(z[cases.NAN_ROW, cases.NAN_COL])
            got = cases.restate(z, y, w, c["classes"], c["icpt"], l2)
            assert np.isnan(got["loss"]) and np.isnan(got["grad"]).all()


@pytest.mark.parametrize("case", cases.FIT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_restatement_under_scipy_is_scikit_learns_fit(case):
    Xtr, ytr, Xte, _ = cases.fit_split(case)
    sk = cases.sklearn_fit(case)
    ours = cases.fit_restated(Xtr.astype(np.float64), ytr, case[5])
    assert np.array_equal(ours["classes"], sk["classes"])
    assert ours["n_iter"] == sk["n_iter"]
    assert (ours["status"] != 0) == (case == cases.CAPPED)
    delta = max(np.abs(ours["coef"] - sk["coef"]).max(), np.abs(ours["intercept"] - sk["intercept"]).max())
    print(f"{case}: n_iter {ours['n_iter']}, max|dcoef| {delta:.3g}, smallest margin {sk['margin'].min():.3g}")
    assert delta < 1e-12
    raw = cases.raw_scores(Xte.astype(np.float64), ours["w"], len(sk["classes"]), True)
    assert np.array_equal(sk["classes"][cases.predict_rule(raw)], sk["pred"])
    assert sk["margin"].min() >= cases.MARGIN


def test_recorded_iteration_counts():
    assert [cases.sklearn_fit(c)["n_iter"] for c in cases.FIT_CASES] == [18, 11, 15, 19, 6, 5, 23]


def test_abi_checks_arguments_and_takes_empty_calls():
    from graphpope_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)                      # host memory: these calls must return before they would touch it
    assert lib.pope_logreg_max_classes() == 64 and lib.pope_logreg_slice_rows() >= 64
    s = lib.pope_logreg_slice_rows()
    assert lib.pope_logreg_scratch_bytes(1000, 128, 7) == 8 * (1000 * 8 + 1000 + -(-1000 // s) * (7 * 129 + 1))
    assert lib.pope_logreg_scratch_bytes(1000, 128, 2) == 8 * (1000 + 1000 + -(-1000 // s) * (129 + 1))
    assert lib.pope_logreg_scratch_bytes(0, 128, 7) == 0 and lib.pope_logreg_scratch_bytes(10, 0, 7) == 0
    assert lib.pope_logreg_scratch_bytes(10, 4, 1) == 0 and lib.pope_logreg_scratch_bytes(10, 4, 65) == 0

    def loss_grad(z=p, ldz=4, n=10, ids=null, m=10, d=4, y=p, classes=3, icpt=1, w=p, loss=p, grad=p, scratch=p, nbytes=1 << 16):
        return lib.pope_logreg_loss_grad(z, ldz, n, ids, m, d, y, classes, icpt, w, 0.1, loss, grad, scratch, nbytes, null)

    def predict(z=p, ldz=4, n=10, ids=null, m=10, d=4, classes=3, icpt=1, w=p, y=null, pred=p, correct=null):
        return lib.pope_logreg_predict(z, ldz, n, ids, m, d, classes, icpt, w, y, pred, correct, null)

    for bad in (dict(z=null), dict(y=null), dict(w=null), dict(loss=null), dict(grad=null), dict(scratch=null), dict(classes=1),
                dict(classes=65), dict(d=0), dict(ldz=3), dict(m=-1), dict(n=0), dict(nbytes=lib.pope_logreg_scratch_bytes(10, 4, 3) - 1)):
        assert loss_grad(**bad) == _lib.ERR_INVALID, bad
        assert b"pope_logreg_loss_grad" in lib.pope_last_error()
    for bad in (dict(z=null), dict(w=null), dict(pred=null), dict(classes=1), dict(classes=65), dict(d=0), dict(ldz=3), dict(m=-1),
                dict(correct=p)):                                  # a count without labels to count against
        assert predict(**bad) == _lib.ERR_INVALID, bad
        assert b"pope_logreg_predict" in lib.pope_last_error()
    # empty calls launch nothing: OK with null pointers, and still refused with bad extents
    assert loss_grad(z=null, y=null, w=null, loss=null, grad=null, scratch=null, nbytes=0, m=0) == _lib.OK
    assert lib.pope_last_error() == b""
    assert predict(z=null, w=null, pred=null, m=0) == _lib.OK
    assert loss_grad(m=0, classes=70) == _lib.ERR_INVALID and predict(m=0, d=0) == _lib.ERR_INVALID
    assert predict(m=0) == _lib.OK and lib.pope_last_error() == b""                 # (clears the error string)


def test_node2vec_test_refuses_what_it_does_not_implement_before_it_needs_a_gpu():
    from graphpope_amd.node2vec import Node2Vec, SecondOrderNode2Vec
    assert SecondOrderNode2Vec.test is Node2Vec.test and SecondOrderNode2Vec.test_nodes is Node2Vec.test_nodes
    model = Node2Vec.__new__(Node2Vec)                         # no constructor: that would need a GPU
    z, y = np.zeros((4, 2), dtype=np.float32), np.arange(4) % 2
    with pytest.raises(NotImplementedError, match="lbfgs"):
        Node2Vec.test(model, z, y, z, y, solver="liblinear")
    with pytest.raises(NotImplementedError, match="auto"):
        Node2Vec.test(model, z, y, z, y, multi_class="ovr")
    with pytest.raises(NotImplementedError, match="max_iter"):
        Node2Vec.test(model, z, y, z, y, penalty="l1")
    with pytest.raises(NotImplementedError, match="positional"):
        Node2Vec.test(model, z, y, z, y, "lbfgs", "auto", 3)
    with pytest.raises(NotImplementedError, match="class_weight"):
        Node2Vec.test_nodes(model, [0, 1], [2, 3], y, class_weight="balanced")


def test_fit_refuses_one_class_before_it_needs_a_gpu():
    import torch
    from graphpope_amd import logreg
    with pytest.raises(ValueError, match="at least 2 classes"):
        logreg.fit(torch.zeros(4, 2), np.zeros(4, dtype=np.int64))
    assert list(logreg._encode(np.array([5, 2, 9, 3]), np.array([2, 5, 9]))) == [1, 0, 2, -1]


def test_generator_eval_flag_defaults_to_off():
    from graphpope_amd import generate_node2vec_embedding as gen
    parser = gen.build_parser()
    assert parser.parse_args([]).eval is False and parser.parse_args(["--eval"]).eval is True
