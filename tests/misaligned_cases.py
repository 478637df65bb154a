"""What every entry point launches for operands that are 4-byte but not 16-byte aligned, and the float64 restatement of the optimiser
step.  Shared by tests/test_misaligned_cpu.py (the tables against the *_kernel_name_at queries, no GPU) and tests/test_misaligned_gpu.py
(the same rows on the device: the name first, then the values).  NumPy only; not a test module.

The strings are tables of outcomes, written down from the launch code (csrc/sage.hip: conv_forward_run, conv_backward_impl; csrc/pairwise.hip:
pairwise_features_impl; csrc/geodesic.hip: finalize_enqueue), for 256 compute units -- not a restatement of the plans' thresholds:
  * forward: one misaligned operand of the projection (agg, w_l, w_r, or the matrix the destination rows are read from) refuses the
    overlapped, whole-tile and stream-K forms, whose loaders move 16 bytes; the plain tile kernel then runs with generic layouts (the two
    products share one instantiation), 64 x 64 tiles at these sizes.  The gather is k_gather_mean<false> when the matrix it reads or one it
    writes is misaligned.  In indexed mode the projection reads x_dst, so a misaligned feature matrix alone only costs the overlapped form
    and the vector gather;
  * backward: grad_out, agg or x misaligned refuse stream-K and k_gemm_dual; the split-K twin of the weight gradients then has generic
    layouts (and the column sums <false> with grad_out).  w_l or w_r misaligned refuse k_gemm_dual and make the grad_x twin generic, but
    leave stream-K alone.  grad_x (and grad_agg, in the scratch) only choose k_scatter_sum_det<false> in deterministic mode;
    k_zero_rows decides inside the kernel.  In indexed mode k_gather_rows copies the destination rows into the (aligned) scratch;
  * pairwise: X or A misaligned refuse the persistent kernel and the vector forms of k_sqnorm / k_pairwise; x or out misaligned turn
    the feature copy into pope_concat in front; out or scratch misaligned turn k_minmax_apply4 into k_minmax_apply;
  * finalise: x (if there is one) or out misaligned: k_finalize<false>."""
import numpy as np

import pairwise_plan_cases as pw
from sage_backward_cases import GENERIC, KC_OC, OC_OC, STREAMK, T64, T128, T256

CUS = 256

# ---- SAGE forward: bits of csrc/sage.hip: FwdAligned ----
F_X, F_AGG, F_OWN, F_XDST, F_WL, F_WR = 1, 2, 4, 8, 16, 32
PLAIN_GENERIC = "k_gemm<%s, %s>" % (T64, GENERIC)
FORWARD_ALIGNED = {
    (4160, 256, 256): "k_gemm_streamk_ld<32>",
    (5800, 256, 256): "k_gather_beside_gemm<3>+k_gemm_tile16<3, 4>",
    (13312, 48, 48): "k_gemm_tile16<4, 4>",
}
# what the one-pass projection is when only the gather's source is misaligned (indexed mode: the projection reads x_dst)
FORWARD_ONE_PASS = {
    (4160, 256, 256): "k_gemm_streamk_ld<32>",
    (5800, 256, 256): "k_gemm_tile16<3, 4>",
    (13312, 48, 48): "k_gemm_tile16<4, 4>",
}
# operand -> (mode "plain" / "indexed", the attribute names to misalign, mask).  `out` and `b_l` are covered by no flag.
FORWARD_OPERANDS = {
    "plain": {"x": F_X | F_OWN, "agg": F_AGG, "w_l": F_WL, "w_r": F_WR, "out": 0, "b_l": 0, "all": F_X | F_OWN | F_AGG | F_WL | F_WR},
    "indexed": {"x": F_X, "agg": F_AGG, "w_l": F_WL, "w_r": F_WR, "out": 0, "b_l": 0, "x_dst": F_OWN | F_XDST, "x_dst_null": 0,
                "all": F_X | F_AGG | F_OWN | F_XDST | F_WL | F_WR},
}


def forward_name(shape, mode, operand):
    mask = FORWARD_OPERANDS[mode][operand]
    if mask == 0:
        return FORWARD_ALIGNED[shape]
    if mask == F_X:                                                   # indexed: the feature matrix alone
        return "k_gather_mean<false>+" + FORWARD_ONE_PASS[shape]
    gather_vec = not mask & (F_X | F_AGG | F_OWN | F_XDST)
    return "k_gather_mean<%s>+%s" % ("true" if gather_vec else "false", PLAIN_GENERIC)


FORWARD_ROWS = [(shape, mode, operand) for shape in FORWARD_ALIGNED for mode in ("plain", "indexed") for operand in FORWARD_OPERANDS[mode]]

# ---- SAGE backward: bits of csrc/sage.hip: BwdAligned, bit 8 = the indexed call ----
B_G, B_AGG, B_X, B_XTMP, B_WL, B_WR, B_GAGG, B_GX, B_INDEXED = 1, 2, 4, 8, 16, 32, 64, 128, 256
BACKWARD_OPERANDS = {"g": B_G, "agg": B_AGG, "x": B_X, "w_l": B_WL, "w_r": B_WR, "grad_x": B_GX, "grad_w_l": 0, "grad_w_r": 0, "grad_b": 0,
                     "all": B_G | B_AGG | B_X | B_WL | B_WR | B_GX}
COLSUM_T, COLSUM_F = "k_colsum_partial<true>", "k_colsum_partial<false>"
TAIL = "+k_scatter_mean"


def _twin(tile, layouts, splits):
    return "k_gemm<%s, %s>" % (tile, layouts) + ("[splits=%d]+k_slab_reduce" % splits if splits > 1 else "")


# shape: (aligned weight-gradient part, splits and tile of the twin that runs when stream-K / dual are refused, grad_x tile)
BACKWARD_SHAPES = {
    (4160, 256, 256): (COLSUM_T + "+" + STREAMK % "[xcd]", 17, T64, T64),
    (4064, 256, 256): ("dual", 16, T64, T64),
    (1030, 40, 24): ("dual", 5, T64, T64),
    (256, 64, 64): (_twin(T64, OC_OC, 1) + "+" + COLSUM_T + "+k_colsum_final", 1, T64, T64),
    (16500, 512, 64): (COLSUM_T + "+" + STREAMK % "[xcd]", 50, T128, T256),
}


def backward_name(shape, operand, extra):
    """sage_conv_backward with both optional gradients and edges, n_src = n_dst + extra, one operand (or all) misaligned."""
    aligned_w, splits, w_tile, x_tile = BACKWARD_SHAPES[shape]
    mask = BACKWARD_OPERANDS[operand]
    zero = "+k_zero_rows" if extra > 0 else ""
    if aligned_w == "dual" and not mask & (B_G | B_AGG | B_X | B_WL | B_WR):
        return "k_gemm_dual<64, 64, 2, 2>[splits=%d]+k_scatter_and_finals" % splits
    if mask & (B_G | B_AGG | B_X):                                   # the weight gradients leave stream-K / dual: generic split-K twin
        w = _twin(w_tile, GENERIC, splits) + "+" + (COLSUM_F if mask & B_G else COLSUM_T) + "+k_colsum_final"
    elif aligned_w == "dual":                                        # w_l / w_r: the twin dual would have run, vector layouts
        w = _twin(w_tile, OC_OC, splits) + "+" + COLSUM_T + "+k_colsum_final"
    else:
        w = aligned_w
    x_layouts = GENERIC if mask & (B_G | B_WL | B_WR) else KC_OC
    return w + zero + "+k_gemm<%s, %s>" % (x_tile, x_layouts) + TAIL


BACKWARD_ROWS = [(shape, operand, extra) for shape in BACKWARD_SHAPES for extra in (0, 300) for operand in BACKWARD_OPERANDS]

# sage_conv_backward_indexed at layer 0 (no input gradient) with the feature matrix misaligned: (mask, name)
INDEXED_SHAPE = (2100, 756, 256)
INDEXED_ALIGNED = (B_INDEXED, COLSUM_T + "+" + STREAMK % "[xcd]")
INDEXED_X = (B_INDEXED | B_X, "k_gather_rows+" + _twin(T128, OC_OC, 9) + "+" + COLSUM_T + "+k_colsum_final")
# no GPU run: the room for the gathered rows lies in the scratch buffer, 256 bytes into it at the least
INDEXED_X_TMP = (B_INDEXED | B_X | B_XTMP, "k_gather_rows+" + _twin(T128, GENERIC, 9) + "+" + COLSUM_T + "+k_colsum_final")

# deterministic mode at (4160, 256, 256), extra 300: (mask, name)
DET_CHAIN = "+k_det_clear+k_det_index<false>+k_det_scan+k_det_index<true>+k_scatter_sum_det<%s>"
DET_SHAPE = (4160, 256, 256)
DET_ROWS = [
    (0, COLSUM_T + "+" + STREAMK % "[xcd]" + "+k_gemm<%s, %s>" % (T64, KC_OC) + DET_CHAIN % "true"),
    (B_GX, COLSUM_T + "+" + STREAMK % "[xcd]" + "+k_gemm<%s, %s>" % (T64, KC_OC) + DET_CHAIN % "false"),
    (B_GAGG, COLSUM_T + "+" + STREAMK % "[xcd]" + "+k_gemm<%s, %s>" % (T64, KC_OC) + DET_CHAIN % "false"),
]

# ---- pairwise: bits of csrc/pairwise.hip: PwAligned; rows of pairwise_plan_cases.CASES ----
P_X, P_A, P_x, P_OUT, P_SCRATCH = 1, 2, 4, 8, 16
PAIRWISE = {
    (257, 128, 256, 8, 1, 0, 0): {P_X: pw.GEN_COPY + pw.FOLD4, P_A: pw.GEN_COPY + pw.FOLD4, P_x: pw.CONCAT + pw.SETS2 + pw.FINISH4,
                                  P_OUT: pw.CONCAT + pw.SETS2 + pw.FINISH1, P_SCRATCH: pw.COPY1 + pw.FINISH1},
    (257, 128, 256, 8, 1, 1, 0): {P_X: pw.GATHER + pw.GEN_COPY + pw.FOLD4, P_A: pw.COPY1 + pw.FINISH4, P_x: pw.CONCAT + pw.SETS2 + pw.FINISH4,
                                  P_OUT: pw.CONCAT + pw.SETS2 + pw.FINISH1, P_SCRATCH: pw.COPY1 + pw.FINISH1},
    (289, 36, 260, 8, 1, 0, 0): {P_X: pw.GEN_COPY + pw.FOLD4, P_A: pw.GEN_COPY + pw.FOLD4, P_x: pw.CONCAT + pw.SETS2 + pw.FINISH4,
                                 P_OUT: pw.CONCAT + pw.SETS2 + pw.FINISH1, P_SCRATCH: pw.COPY1 + pw.FINISH1},
    (257, 132, 256, 8, 1, 0, 0): {P_X: pw.GEN_COPY + pw.FOLD4, P_A: pw.GEN_COPY + pw.FOLD4, P_x: pw.CONCAT + pw.VEC + pw.FOLD4,
                                  P_OUT: pw.CONCAT + pw.VEC + pw.FOLD1, P_SCRATCH: pw.VEC_COPY + pw.FOLD1},
    # no GPU run (its knob is not 0): the gathered anchor rows lie in the scratch
    (257, 128, 256, 8, 1, 1, 1): {P_SCRATCH: pw.GATHER + pw.GEN_COPY + pw.FOLD1},
}
PAIRWISE_GPU_ROWS = [row for row in PAIRWISE if row[6] == 0]
# The scratch holds float2 pairs of row norms: its base needs 8 bytes at the least, so a 4-byte offset is not a supported input and
# bit P_SCRATCH stays with the CPU table.
PAIRWISE_GPU_BITS = {"X": P_X, "A": P_A, "x": P_x, "out": P_OUT}

# ---- geodesic finalise: bit 0 = x, bit 1 = out; (N, K, F) of the GPU run ----
FINALIZE_SHAPE = (2048, 64, 8)
FINALIZE = {(1, 0): "k_finalize_pipe<1, 1>", (1, 1): "k_finalize<false>", (1, 2): "k_finalize<false>", (1, 3): "k_finalize<false>",
            (0, 0): "k_finalize_pipe<0, 1>", (0, 1): "k_finalize_pipe<0, 1>", (0, 2): "k_finalize<false>"}      # (has_x, mask)

# what each family's table must show at least once (the right-hand column of the plans' alignment inputs)
ALTERNATIVES = {
    "forward": ["k_gather_mean<false>", "k_gather_mean<true>+" + PLAIN_GENERIC, "k_gather_mean<false>+k_gemm_tile16", "k_gather_mean<false>+k_gemm_streamk_ld"],
    "backward": ["k_gemm<%s, %s>[splits=" % (T64, GENERIC), "k_gemm<%s, %s>[splits=50]" % (T128, GENERIC), COLSUM_F,
                 STREAMK % "[xcd]" + "+k_gemm<%s, %s>" % (T256, GENERIC), "k_gemm<%s, %s>[splits=16]" % (T64, OC_OC), "k_gather_rows+",
                 "k_scatter_sum_det<false>"],
    "pairwise": ["k_sqnorm<false>+k_pairwise<0>", "pope_concat+", "k_minmax_apply", "k_gather_anchor_rows+k_sqnorm<false>"],
    "finalize": ["k_finalize<false>"],
}

# ---- the optimiser: one step of csrc/epilogue.hip: k_adam's update() restated in float64, and what float32 may differ by ----
ADAM_LENGTHS = [1, 3, 4, 4095, 4096, 4099, 7 * 256]                   # around ADAM_CHUNK = 4096, the pack of four and the block of 256
U = 2.0 ** -24                                                        # unit roundoff of float32


def adam_reference(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, coef=None):
    """One step from the float32 state (p, g, m, v) with the float32 scalars the library forms (sage_adam_step: lr / (1 - beta1^t) and
    1 / sqrt(1 - beta2^t) in double, rounded once; 1 - beta rounded from double), every operation of update() in float64:
        G  = g * coef + wd * p               m' = m + (G - m) * (1 - beta1)          v' = beta2 * v + (1 - beta2) * G * G
        p' = p - s * (m' / (sqrt(v') * c + eps))
    and the bound on |float32 result - this| that follows from counting the roundings of update(), each relative error at most u = 2^-24
    (a fused multiply-add rounds once where the count below has two, and HIP's float32 division and square root are correctly rounded,
    counted here as 2 u each so that a 1-ulp implementation passes as well):
        E_G  = u (|g coef| + |wd p| + |G|)                                  two products, one sum
        E_m  = a E_G + 2 u a (|G| + |m|) + u |m'|                           G - m, * a, m + .        (a = 1 - beta1)
        E_v  = u b |v| + c2 (2 |G| E_G + 2 u G^2) + u |v'|                  b v; c2 G, * G; the sum
        E_sq = E_v / (2 sqrt(v')) + 2 u sqrt(v')                            the argument's error through the root, the root itself
        E_D  = c E_sq + u c sqrt(v') + u D                                  * c, + eps               (D = sqrt(v') c + eps)
        E_r  = E_m / D + |m'| E_D / D^2 + 2 u |r|                           numerator, denominator, the division   (r = m' / D)
        E_p  = s E_r + u s |r| + u |p'|                                     * s, p - .
    to first order in u; the factor 1 + 2^-10 on every bound covers the second-order terms (each is below 64 u times a first-order one).
    Returns ({p, m, v}: float64 values, {p, m, v}: bounds).  A NaN gradient element makes its own p', m', v' NaN and nothing else."""
    f32, f64 = np.float32, np.float64
    s = f64(f32(lr / (1.0 - beta1 ** step)))
    c = f64(f32(1.0 / np.sqrt(1.0 - beta2 ** step)))
    a, b, c2, e, wd = f64(f32(1.0 - beta1)), f64(f32(beta2)), f64(f32(1.0 - beta2)), f64(f32(eps)), f64(f32(weight_decay))
    k = f64(1.0) if coef is None else f64(f32(coef))
    p, g, m, v = (x.astype(f64) for x in (p, g, m, v))
    G = g * k + wd * p
    m1 = m + (G - m) * a
    v1 = b * v + c2 * G * G
    root = np.sqrt(v1)
    D = root * c + e
    r = m1 / D
    p1 = p - s * r
    with np.errstate(invalid="ignore", divide="ignore"):
        E_G = U * (np.abs(g * k) + np.abs(wd * p) + np.abs(G))
        E_m = a * E_G + 2 * U * a * (np.abs(G) + np.abs(m)) + U * np.abs(m1)
        E_v = U * b * np.abs(v) + c2 * (2 * np.abs(G) * E_G + 2 * U * G * G) + U * np.abs(v1)
        E_sq = np.where(v1 > 0, E_v / (2 * np.where(v1 > 0, root, 1.0)), 0.0) + 2 * U * root
        E_D = c * E_sq + U * c * root + U * D
        E_r = E_m / D + np.abs(m1) * E_D / (D * D) + 2 * U * np.abs(r)
        E_p = s * E_r + U * s * np.abs(r) + U * np.abs(p1)
    slack = 1.0 + 2.0 ** -10
    return dict(p=p1, m=m1, v=v1), dict(p=E_p * slack, m=E_m * slack, v=E_v * slack)


def clip_coefficient(norm64, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in float64 from the float64 norm, and the relative error the float32 coefficient may have: the
    norm rounded to float32, the sum with float32(1e-6), the division, max_norm rounded to float32, 1e-6 itself rounded -- 5 u."""
    c = float(max_norm) / (float(norm64) + 1e-6)
    return min(1.0, c), 5 * U


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements that are numbers on both sides; an exact element counts 0 whatever its bound."""
    ok = ~(np.isnan(got) | np.isnan(want))
    err = np.abs(got.astype(np.float64) - want)[ok]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound[ok])
    return float(ratio.max()) if ratio.size else 0.0
