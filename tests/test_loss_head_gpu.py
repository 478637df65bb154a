"""The training loss head on the GPU (csrc/epilogue.hip: k_xent_rows, k_xent_final, the loss block of k_adam) against the NumPy
float64 reference and the float32-rounding bounds of tests/loss_head_cases.py -- main.py:216 F.cross_entropy(y_hat, y).

Every case runs through the library's own entry points (raw pointers), in each of the forms a training step can take:
  1  fused = 0, then sage_cross_entropy_backward with an upstream gradient of 1.7
  2  fused = 1
  3  fused = 2, finished by sage_adam_step_loss with no tensor (the k_xent_final fallback)
  4  fused = 2, finished by the loss block of k_adam<false> (one small parameter tensor)
  5  fused = 2, finished by sage_adam_step_clip (k_adam<true>)
  6  form 4 with 27 parameter tensors: two launches, only the first carries the loss block
Each test prints its worst error-to-bound ratios (DESIGN.md records them)."""
import ctypes

import numpy as np
import pytest
import torch

import loss_head_cases as lh

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
FORM_NAMES = {1: "unfused + backward", 2: "fused", 3: "fused, k_xent_final fallback", 4: "fused, k_adam<false>", 5: "fused, k_adam<true>",
              6: "fused, k_adam<false> x 27 tensors"}


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


def _finish_with_adam(lib, dev, stream, rows, n, out, n_tensors, clip):
    """One Adam step (step 1, zero moments) over n_tensors identical 5-element tensors whose launch finishes the loss; checks the step."""
    from graphpope_amd._lib import check, ptr
    lr = 1e-2
    p0 = torch.tensor([0.5, -0.25, 1.0, 2.0, -3.0], device=dev)
    g0 = torch.tensor([0.1, -0.2, 0.3, -0.4, 0.5], device=dev)
    ps = [p0.clone() for _ in range(n_tensors)]
    gs = [g0.clone() for _ in range(n_tensors)]
    ms = [torch.zeros(5, device=dev) for _ in range(n_tensors)]
    vs = [torch.zeros(5, device=dev) for _ in range(n_tensors)]
    arr = ctypes.c_void_p * n_tensors
    pp, gg, mm, vv = (arr(*[t.data_ptr() for t in ts]) for ts in (ps, gs, ms, vs))
    nn = (ctypes.c_int64 * n_tensors)(*([5] * n_tensors))
    if clip:
        parts = int(lib.sage_grad_norm_partials(n_tensors, nn))
        ws = torch.zeros(256, dtype=torch.float64, device=dev)
        norm = torch.zeros(2, device=dev)
        check(lib.sage_grad_sqnorm(n_tensors, gg, nn, ptr(ws), parts, stream))
        check(lib.sage_adam_step_clip(n_tensors, pp, gg, mm, vv, nn, lr, 0.9, 0.999, 1e-8, 0.0, 1, None, 0.5, ptr(ws), parts, ptr(norm),
                                      ptr(rows), n, ptr(out), stream))
    else:
        check(lib.sage_adam_step_loss(n_tensors, pp, gg, mm, vv, nn, lr, 0.9, 0.999, 1e-8, 0.0, 1, None, ptr(rows), n, ptr(out), stream))
    want = p0 - lr * torch.sign(g0)                                   # step 1 from zero moments: m / sqrt(v) = sign(g), whatever scales g
    for p in ps:
        assert float((p - want).abs().max()) < 1e-5
    if clip:
        total = float(np.sqrt(n_tensors * float((g0.double() ** 2).sum())))
        assert abs(float(norm[0]) - total) <= 1e-6 * total


def run_form(lib, dev, case, ref, form):
    """One form of the loss head on `case`; returns the dict tests/loss_head_cases.check takes."""
    from graphpope_amd._lib import check, ptr
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, c = case.logits.shape
    logits = torch.as_tensor(case.logits, device=dev)
    y = torch.as_tensor(case.y, device=dev)
    out = torch.full((2,), SENTINEL, device=dev)                      # (loss, 1 / count) of sage_cross_entropy_forward
    grad = torch.full((n, c), SENTINEL, device=dev)
    rows = torch.full((n,), SENTINEL, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    fused = {1: 0, 2: 1}.get(form, 2)
    check(lib.sage_cross_entropy_forward(ptr(logits), ptr(y), n, c, case.ignore_index, ptr(out), ptr(grad), ctypes.c_void_p(out.data_ptr() + 4),
                                         ptr(rows), ptr(bad), fused, stream))
    got = {}
    if form == 1:
        up = torch.tensor([lh.UPSTREAM], device=dev)
        scaled = torch.full((n, c), SENTINEL, device=dev)
        check(lib.sage_cross_entropy_backward(ptr(grad), n, c, ptr(up), ctypes.c_void_p(out.data_ptr() + 4), ptr(scaled), stream))
        got.update(grad_scale=1.0, scaled=scaled.cpu().numpy(),
                   scaled_scale=float(np.float32(lh.UPSTREAM)) / ref.count if ref.count else 0.0)
    else:
        got.update(grad_scale=1.0 / ref.count if ref.count else 0.0)
    if form >= 3:
        assert out.tolist() == [SENTINEL, SENTINEL]                    # fused = 2 writes neither scalar
        fin = torch.full((2,), SENTINEL, device=dev)
        if form == 3:
            check(lib.sage_adam_step_loss(0, None, None, None, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, 1, None, ptr(rows), n, ptr(fin), stream))
        else:
            _finish_with_adam(lib, dev, stream, rows, n, fin, 27 if form == 6 else 1, clip=form == 5)
        out = fin
    o = out.cpu().numpy()
    got.update(loss=float(o[0]), inv_count=o[1], bad=int(bad), rows=rows.cpu().numpy(), grad=grad.cpu().numpy())
    return got


def _run_family(dev, cases, title):
    from graphpope_amd import _lib
    lib = _lib.load()
    worst = {}
    failures = []
    for case in cases:
        ref = lh.reference(case.logits, case.y, case.ignore_index)
        for form in case.forms:
            try:
                lh.merge(worst.setdefault(form, {}), lh.check(case, ref, run_form(lib, dev, case, ref, form), FORM_NAMES[form]))
            except AssertionError as e:                                # every case and form is reported, not only the first
                failures.append(str(e)[:300])
    for form in sorted(worst):
        print(f"{title}: form {form} ({FORM_NAMES[form]}): " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst[form].items())))
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:12])
    return worst


def test_every_column_count_and_the_switch_between_the_two_row_forms(dev):
    """C in {1, 2, 63, 64, 65, 448, 511, 512, 513, 1000, 1025}: the register form up to 512 columns, the looped form above; at
    (257, 513) all six forms."""
    worst = _run_family(dev, lh.column_cases(), "columns")
    assert set(worst) == {1, 2, 3, 4, 5, 6}


def test_row_counts_around_the_strides_of_the_count_loop_and_the_final_block(dev):
    """N in {1, 3, 4, 5, 255 .. 257, 2047 .. 2049, 4097, 16390} at C = 3, the rows at the edges of every 256-row stride alternately
    ignored and counted: 1 / count equals float32(1) / float32(count) exactly in every form."""
    _run_family(dev, lh.row_cases(), "rows")


def test_magnitudes_shifts_and_confident_rows(dev):
    """Logits scaled by 1e-3 .. 3e3, constant rows, rows shifted by -1e6 and +3e4, a label column that leads by 30 (row loss exactly
    +0 and still counted: the "not counted" marker is negative) or trails by 200 (softmax exactly 0 at the label)."""
    _run_family(dev, lh.magnitude_cases(), "magnitude")


def test_ignore_index_inside_the_range_bad_labels_and_nothing_counted(dev):
    _run_family(dev, lh.label_cases(), "labels")


def test_non_finite_logits_poison_what_torch_poisons(dev):
    """A NaN or +inf logit in a counted row, or a row of -inf, makes the mean loss NaN in every form while 1 / count stays 1 / (rows
    counted by label); -inf at the label gives +inf; in an ignored row, or at another column as -inf, it changes nothing."""
    _run_family(dev, lh.non_finite_cases(), "non-finite")


def test_row_terms_are_the_evaluation_kernels(dev):
    """include/graphpope_hip.h: sage_eval_metrics forms its terms "exactly as sage_cross_entropy_forward forms" them.  Its loss sum
    against the float64 sum of the counted row_scratch entries: only the order of the float64 additions may differ."""
    from graphpope_amd import _lib
    from graphpope_amd.sage import EvalMetrics
    lib = _lib.load()
    for case in lh.eval_agreement_cases():
        ref = lh.reference(case.logits, case.y)
        terms = run_form(lib, dev, case, ref, 1)["rows"].astype(np.float64)[ref.counted]
        metrics = EvalMetrics(dev)
        metrics.update(torch.as_tensor(case.logits, device=dev), torch.as_tensor(case.y, device=dev))
        w = metrics.acc.cpu().numpy()
        loss_sum, rows = float(w[:1].view(np.float64)[0]), int(w[2])
        tol = case.y.size * 2.0 ** -53 * float(np.abs(terms).sum())
        print(f"{case.name}: eval {loss_sum!r} vs rows {float(terms.sum())!r}, tolerance {tol:.3g}")
        assert rows == ref.count == terms.size
        assert abs(loss_sum - float(terms.sum())) <= tol
