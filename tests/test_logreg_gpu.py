"""Logistic regression on the GPU (csrc/logreg.hip, graphpope_amd.logreg, ``Node2Vec.test``): the objective against the longdouble
restatement within the derived bounds of tests/logreg_cases.py, its bit-reproducibility, the predictions, the fit against
scikit-learn's on the float64 copy of the same rows, and an end-to-end run that shows training puts graph structure into the table."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import logreg_cases as cases
from conftest import ROOT

pytestmark = pytest.mark.gpu

PARITY = os.path.join(ROOT, "profiles", "logreg_parity.json")


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


def _np(a):
    return torch.from_numpy(np.array(a))                                      # (a copy: the cases' arrays are read-only)


def _lib():
    from graphpope_amd import _lib as binding
    return binding, binding.load()


def _stream():
    from graphpope_amd import engine
    return engine._stream()


def _objective(dev, case, materialise=False, poison=False):
    """(loss float64, grad float64 [P]) of pope_logreg_loss_grad on a case: the table with its padded row stride and, for an ids
    case, the ids -- or, ``materialise``, the selected rows copied out densely."""
    binding, lib = _lib()
    table, sel, z, y, w, l2 = cases.objective_inputs(case)
    m, d, classes = case["m"], case["d"], case["classes"]
    if materialise:
        zt, ids, ldz = _np(np.ascontiguousarray(z)).to(dev), None, d
    else:
        zt, ids, ldz = _np(table).to(dev), (None if sel is None else _np(sel).to(dev)), table.shape[1]
    yt = _np(y.astype(np.int32)).to(dev)
    wt = _np(w).to(dev)
    out = torch.full((1 + w.size,), 7.0, dtype=torch.float64, device=dev)
    need = lib.pope_logreg_scratch_bytes(m, d, classes)
    assert need > 0
    scratch = torch.full((need // 8,), float("nan") if poison else 0.0, dtype=torch.float64, device=dev)
    binding.check(lib.pope_logreg_loss_grad(binding.ptr(zt), ldz, zt.shape[0], binding.ptr(ids), m, d, binding.ptr(yt), classes, int(case["icpt"]),
                                            binding.ptr(wt), l2, binding.ptr(out), binding.c_void_p(out.data_ptr() + 8), binding.ptr(scratch),
                                            need, _stream()))
    res = out.cpu().numpy()
    return res[0], res[1:]


def _predict(dev, z, w, classes, icpt, y=None):
    """(pred int32 [m], correct or None) of pope_logreg_predict on dense rows."""
    binding, lib = _lib()
    zt = _np(np.ascontiguousarray(z)).to(dev)
    m, d = zt.shape
    wt = _np(np.ascontiguousarray(w)).to(dev)
    pred = torch.full((m,), -7, dtype=torch.int32, device=dev)
    yt = None if y is None else _np(y.astype(np.int32)).to(dev)
    correct = None if y is None else torch.full((1,), 12345, dtype=torch.int64, device=dev)
    binding.check(lib.pope_logreg_predict(binding.ptr(zt), d, m, None, m, d, classes, int(icpt), binding.ptr(wt), binding.ptr(yt),
                                          binding.ptr(pred), binding.ptr(correct), _stream()))
    return pred.cpu().numpy(), (None if correct is None else int(correct))


def _table(dev):
    _, lib = _lib()
    return cases.objective_cases(lib.pope_logreg_slice_rows())


# ---- pope_logreg_loss_grad ------------------------------------------------------------------------------------------------------------
def test_loss_and_gradient_stay_within_the_derived_bounds(dev):
    table = _table(dev)
    slice_rows = _lib()[1].pope_logreg_slice_rows()
    assert any(c["m"] > 2 * slice_rows and c["m"] % slice_rows for c in table)           # three slices, the last one ragged
    worst = []
    for c in table:
        loss, grad = _objective(dev, c)
        ref, lb, gb = cases.reference(c)
        if c["nan"]:
            want = np.isnan(np.asarray(ref["grad"], dtype=np.float64))
            assert np.isnan(ref["loss"]) and want.all()
            assert np.isnan(loss) and (np.isnan(grad) == want).all(), c["id"]
            continue
        el = abs(float(np.longdouble(loss) - ref["loss"]))
        eg = np.abs((grad.astype(np.longdouble) - ref["grad"]).astype(np.float64))
        worst.append((max(el / lb, float((eg / gb).max())), el / lb, float((eg / gb).max()), c["id"]))
    worst.sort(reverse=True)
    print(f"{len(worst)} cases; largest error / bound {worst[0][0]:.3g} ({worst[0][3]}: loss {worst[0][1]:.3g}, gradient {worst[0][2]:.3g}); "
          f"next {worst[1][0]:.3g} ({worst[1][3]})")
    bad = [w for w in worst if not w[0] <= 1.0]
    assert not bad, bad[:5]


def test_two_calls_give_the_same_bits_whatever_the_scratch_held(dev):
    for c in _table(dev):
        if c["nan"] or c["w"] == "zero":
            continue
        a, b = _objective(dev, c), _objective(dev, c, poison=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), c["id"]


def test_rows_selected_by_id_give_the_bits_of_the_rows_copied_out(dev):
    seen = 0
    for c in _table(dev):
        if c["ids"] or c["pad"]:
            a, b = _objective(dev, c), _objective(dev, c, materialise=True)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), c["id"]
            seen += bool(c["ids"])
    assert seen >= 4


def test_a_row_outside_the_table_is_not_read(dev):
    """ids beyond N: the row counts as NaN (loss NaN) instead of being fetched."""
    binding, lib = _lib()
    z = torch.zeros(4, 3, device=dev)
    ids = torch.tensor([0, 9, -1, 2], device=dev)
    y = torch.zeros(4, dtype=torch.int32, device=dev)
    w = torch.zeros(3 * 4, dtype=torch.float64, device=dev)
    out = torch.zeros(1 + 12, dtype=torch.float64, device=dev)
    scratch = torch.zeros(lib.pope_logreg_scratch_bytes(4, 3, 3) // 8, dtype=torch.float64, device=dev)
    binding.check(lib.pope_logreg_loss_grad(binding.ptr(z), 3, 4, binding.ptr(ids), 4, 3, binding.ptr(y), 3, 1, binding.ptr(w), 0.25, binding.ptr(out),
                                            binding.c_void_p(out.data_ptr() + 8), binding.ptr(scratch), scratch.numel() * 8, _stream()))
    assert torch.isnan(out).all()


# ---- pope_logreg_predict --------------------------------------------------------------------------------------------------------------
def test_predictions_follow_the_argmax_and_sign_rules(dev):
    rows = 0
    for c in _table(dev):
        if c["nan"]:
            continue
        table, sel, z, y, w, _ = cases.objective_inputs(c)
        raw = np.asarray(cases.reference(c)[0]["raw"], dtype=np.float64)
        want = cases.predict_rule(raw)
        if c["w"] == "zero":
            assert not raw.any() and not want.any()                          # every class ties at 0: the first index, and 0 > 0 is false
        else:                                                                 # no near-tie among these rows: the rule decides every one
            gap = np.abs(raw[:, 0]) if raw.shape[1] == 1 else np.sort(raw, axis=1)[:, -1] - np.sort(raw, axis=1)[:, -2]
            assert gap.min() > 1e-9 * (1 + np.abs(raw).max()), c["id"]
        binding, lib = _lib()
        zt = _np(table).to(dev)
        it = None if sel is None else _np(sel).to(dev)
        wt = _np(w).to(dev)
        yt = _np(y.astype(np.int32)).to(dev)
        pred = torch.full((c["m"],), -7, dtype=torch.int32, device=dev)
        correct = torch.full((1,), 12345, dtype=torch.int64, device=dev)
        binding.check(lib.pope_logreg_predict(binding.ptr(zt), table.shape[1], table.shape[0], binding.ptr(it), c["m"], c["d"], c["classes"],
                                              int(c["icpt"]), binding.ptr(wt), binding.ptr(yt), binding.ptr(pred), binding.ptr(correct), _stream()))
        got = pred.cpu().numpy()
        assert np.array_equal(got, want), c["id"]
        assert int(correct) == int((want == y).sum()), c["id"]
        rows += c["m"]
    assert rows > 5000


def test_an_exact_tie_goes_to_the_first_class_and_an_unseen_label_never_counts(dev):
    rng = np.random.default_rng(7)
    m, d, classes = 333, 33, 4
    z = np.float32(rng.standard_normal((m, d)))
    table = rng.standard_normal((classes, d + 1))
    table[3] = table[1]                                                       # classes 1 and 3 tie exactly on every row
    table[1:4:2, d] += 2.0                                                    # ... and win most of them
    w = table.ravel(order="F")
    raw = cases.raw_scores(z, w, classes, True)
    raw[:, 3] = raw[:, 1]
    want = cases.predict_rule(raw)
    others = np.sort(raw[:, [0, 1, 2]], axis=1)
    assert (others[:, -1] - others[:, -2]).min() > 1e-9 and (want == 1).sum() > m // 3 and not (want == 3).any()
    y = rng.integers(0, classes, m)
    y[::5] = -1                                                               # labels no training row had
    y[1::5] = want[1::5]
    got, correct = _predict(dev, z, w, classes, True, y=y)
    assert np.array_equal(got, want)
    assert correct == int((want == y).sum()) and 0 < correct < m and (y == -1).sum() > 60
    got, correct = _predict(dev, z, w, classes, True, y=np.full(m, -1))
    assert np.array_equal(got, want) and correct == 0
    got, correct = _predict(dev, z, w, classes, True)                         # no labels: predictions alone
    assert np.array_equal(got, want) and correct is None


# ---- logreg.fit / score ---------------------------------------------------------------------------------------------------------------
_FITS = {}


def _device_fit(dev, case):
    """(model, score, predictions, warned) of logreg.fit on a fit case, computed once."""
    if case not in _FITS:
        from sklearn.exceptions import ConvergenceWarning
        from graphpope_amd import logreg
        Xtr, ytr, Xte, yte = cases.fit_split(case)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            model = logreg.fit(_np(Xtr), ytr, max_iter=case[5])
        warned = [w for w in caught if issubclass(w.category, ConvergenceWarning)]
        assert len(warned) == len(caught)
        zte = _np(Xte)
        _FITS[case] = (model, logreg.score(model, zte, yte), logreg.predict(model, zte), bool(warned))
    return _FITS[case]


@pytest.mark.parametrize("case", cases.FIT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_fit_follows_scikit_learn(dev, case):
    model, score, pred, warned = _device_fit(dev, case)
    sk = cases.sklearn_fit(case)
    d, n_cls = case[1], len(sk["classes"])
    assert np.array_equal(model.classes_, sk["classes"])
    assert model.coef_.shape == sk["coef"].shape == (1 if n_cls == 2 else n_cls, d) and model.intercept_.shape == sk["intercept"].shape
    assert model.coef_.dtype == np.float64 and model.n_iter_.shape == (1,)
    delta = max(np.abs(model.coef_ - sk["coef"]).max(), np.abs(model.intercept_ - sk["intercept"]).max())
    print(f"{case}: n_iter {int(model.n_iter_[0])} (scikit-learn {sk['n_iter']}), max|dcoef| {delta:.3g}, score {score!r} ({sk['score']!r}), "
          f"smallest margin {sk['margin'].min():.3g}")
    assert warned == (case == cases.CAPPED)                                   # the iteration cap warns, and is no error
    assert isinstance(score, float) and score == sk["score"]
    clear = sk["margin"] >= cases.MARGIN
    assert (~clear).sum() <= cases.EXCUSED * len(clear)
    assert np.array_equal(pred[clear], sk["pred"][clear])


def test_coefficients_stay_within_the_recorded_parity(dev):
    """n_iter_ and max|dcoef| against scikit-learn per fit case; profiles/logreg_parity.json holds the values of the first GPU run
    (written here when the file is missing).  Asserted: 100 x the largest recorded value (order-dependent amplification across
    L-BFGS iterations), with a ceiling of 1e-9 that float32 accumulation would miss by orders of magnitude."""
    measured = []
    for case in cases.FIT_CASES:
        model, *_ = _device_fit(dev, case)
        sk = cases.sklearn_fit(case)
        delta = max(np.abs(model.coef_ - sk["coef"]).max(), np.abs(model.intercept_ - sk["intercept"]).max())
        measured.append(dict(case=list(case), n_iter=int(model.n_iter_[0]), n_iter_sklearn=sk["n_iter"], max_abs_dcoef=float(delta)))
    if not os.path.exists(PARITY):
        with open(PARITY, "w") as f:
            json.dump(dict(reference="scikit-learn LogisticRegression(solver='lbfgs') on the float64 copy", cases=measured), f, indent=1)
            f.write("\n")
    recorded = json.load(open(PARITY))["cases"]
    assert [r["case"] for r in recorded] == [list(c) for c in cases.FIT_CASES]
    largest = max(r["max_abs_dcoef"] for r in recorded)
    assert largest <= cases.COEF_CEILING                                      # a recorded value above the ceiling is a finding
    bound = min(100 * largest, cases.COEF_CEILING)
    print(f"recorded largest max|dcoef| {largest:.3g}: bound {bound:.3g}; measured {[(m['n_iter'], m['n_iter_sklearn'], m['max_abs_dcoef']) for m in measured]}")
    for got in measured:
        assert got["max_abs_dcoef"] <= bound, got


def test_fit_refuses_non_finite_rows_and_ids_outside_the_table(dev):
    from graphpope_amd import logreg
    Xtr, ytr, _, _ = cases.fit_split(cases.FIT_CASES[3])
    z = _np(Xtr.copy())
    z[5, 2] = float("inf")
    with pytest.raises(ValueError, match="NaN or infinity"):
        logreg.fit(z, ytr)
    ids = np.array([i for i in range(len(ytr)) if i != 5])
    assert logreg.fit(z, ytr[ids], ids=ids).n_iter_[0] > 0                    # the bad row is not among the selected ones
    with pytest.raises(IndexError):
        logreg.fit(z, ytr[:3], ids=[0, 1, len(ytr)])
    with pytest.raises(TypeError):
        logreg.fit(z.double(), ytr)


# ---- Node2Vec.test / test_nodes -------------------------------------------------------------------------------------------------------
def _planted_model(dev):
    from graphpope_amd.node2vec import Node2Vec
    ei, labels = cases.planted_partition()
    torch.manual_seed(0)
    model = Node2Vec(torch.as_tensor(ei, device=dev), 32, walk_length=10, context_size=5, walks_per_node=4, num_nodes=len(labels))
    nodes = np.arange(len(labels))
    return model, labels, nodes[nodes % 2 == 0], nodes[nodes % 2 == 1]


def test_node2vec_test_and_test_nodes_are_the_same_fit(dev):
    from graphpope_amd import logreg
    model, labels, train, test = _planted_model(dev)
    z, y = model.embedding.weight.detach(), torch.as_tensor(labels)
    a = model.test(z[train], y[train], z[test], y[test], max_iter=150)
    b = model.test_nodes(train, test, labels, max_iter=150)
    c = model.test(z[train].cpu(), y[train].to(dev), z[test].cpu(), y[test].numpy(), "lbfgs", "auto", max_iter=150)
    fitted = logreg.fit(z[train], labels[train], max_iter=150)
    by_ids = logreg.fit(z, labels[train], ids=train, max_iter=150)
    assert fitted.w.tobytes() == by_ids.w.tobytes() and fitted.n_iter_[0] == by_ids.n_iter_[0]
    assert isinstance(a, float) and a == b == c == logreg.score(fitted, z[test], labels[test])
    from sklearn.linear_model import LogisticRegression
    zc = z.cpu().numpy().astype(np.float64)
    assert a == LogisticRegression(max_iter=150).fit(zc[train], labels[train]).score(zc[test], labels[test])


def test_training_puts_the_communities_into_the_table(dev):
    """4 communities x 64 nodes, p_in / p_out = 60: the untrained table scores at most chance + 4 sigma of a binomial over the 128
    test nodes, 0.25 + 4 sqrt(0.25 * 0.75 / 128) = 0.403; the trained one at least 0.625, halfway between chance and 1."""
    from graphpope_amd.sage import deterministic
    model, labels, train, test = _planted_model(dev)
    with deterministic(True):
        before = model.test_nodes(train, test, labels, max_iter=150)
        losses = model.fit(epochs=8, batch_size=64, lr=0.05, seed=0)
        after = model.test_nodes(train, test, labels, max_iter=150)
    print(f"planted partition: accuracy untrained {before:.4f}, after 8 epochs {after:.4f}; epoch losses {[round(x, 3) for x in losses]}")
    assert before <= 0.25 + 4 * np.sqrt(0.25 * 0.75 / 128)
    assert after >= 0.625


# ---- the generator --------------------------------------------------------------------------------------------------------------------
def test_generator_eval_prints_accuracies_and_saves_the_same_table(dev, tmp_path, monkeypatch, capsys):
    import re
    from graphpope_amd import generate_node2vec_embedding as gen
    ei, labels = cases.planted_partition()
    n = len(labels)
    even = np.arange(n) % 2 == 0
    np.savez(tmp_path / "pubmed.npz", x=np.zeros((n, 4), dtype=np.float32), y=labels, edge_index=ei, train_mask=even, val_mask=~even,
             test_mask=~even)
    monkeypatch.setenv("GRAPHPOPE_DETERMINISTIC", "1")
    common = ["--dataset", "pubmed", "--data_dir", str(tmp_path), "--embedding_dim", "32", "--walk_length", "10", "--context_size", "5",
              "--walks_per_node", "2", "--batch_size", "64"]
    capsys.readouterr()
    gen.main(common + ["--epochs", "2", "--out", str(tmp_path / "plain.pt")])
    plain = capsys.readouterr().out.splitlines()
    gen.main(common + ["--epochs", "2", "--eval", "--out", str(tmp_path / "eval.pt")])
    with_eval = capsys.readouterr().out.splitlines()
    gen.main(common + ["--epochs", "0", "--eval", "--out", str(tmp_path / "untrained.pt")])
    untrained = capsys.readouterr().out.splitlines()
    assert len(plain) == len(with_eval) == 4 and len(untrained) == 3
    for e in (0, 1):
        assert re.fullmatch(rf"epoch {e}: loss \d+\.\d{{4}}", plain[1 + e])
        assert re.fullmatch(rf"epoch {e}: loss \d+\.\d{{4}} acc [01]\.\d{{4}}", with_eval[1 + e]) and with_eval[1 + e].startswith(plain[1 + e])
    assert re.fullmatch(r"untrained: acc [01]\.\d{4}", untrained[1])
    assert plain[0] == with_eval[0] and plain[-1] == with_eval[-1]
    a, b = torch.load(tmp_path / "plain.pt"), torch.load(tmp_path / "eval.pt")
    assert a.shape == (n, 32) and torch.equal(a.view(torch.int32), b.view(torch.int32))
