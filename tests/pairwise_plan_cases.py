"""What the node2vec-space call launches, shape by shape (csrc/pairwise.hip: pairwise_plan), NumPy only.

CASES rows are (n, d, k, f, has_x, by_id, knob) -> the string pope_pairwise_kernel_name must print on CUS compute units: the launches in
order, under the query's assumptions (16-byte-aligned bases, c0 = f, out_cols = f + k, a side-stream slot).  The strings were written down
from the launch code as it stood before the plan existed (one `if` per decision, spread over five functions), not from the query:
  * the persistent kernel takes d <= 128, d % 4 == 0, n * (f + k) * 4 < 2^32, unless the knob is 1; consumer sets: 1 beside the side copy,
    else 2; knob 2 / 3 force 1 / 2;
  * the feature copy wants f % 4 == 0 and (f + k) % 4 == 0, else pope_concat runs first; beside the persistent kernel also f <= 4096
    (else pope_concat), while the one-tile kernel carries any width;
  * the one-tile kernel's operands are vectors (k_sqnorm<true>, k_pairwise<1>) when d % 4 == 0, else generic (<false>, <0>); anchors given
    as ids are gathered in front of it;
  * the scaling pass is k_minmax_apply4 when k, f and f + k are multiples of 4.
Used by test_abi.py (the whole table, no GPU), test_pairwise_plan_gpu.py (rows with n <= GPU_MAX_N: values against float64) and
tools/pairwise_bits.py.  SCRATCH_SHAPES is the table of tests/golden/pairwise_scratch_sizes.json (tools/pairwise_scratch_sizes.py).
"""
import functools

import numpy as np

import pairwise_cases as pc

CUS = 256
GPU_MAX_N = 600

FINISH4, FINISH1 = "k_minmax_finish+k_minmax_apply4", "k_minmax_finish+k_minmax_apply"
FOLD4, FOLD1 = "k_minmax_fold+k_minmax_reduce+k_minmax_apply4", "k_minmax_fold+k_minmax_reduce+k_minmax_apply"
SETS2, SETS1 = "k_pairwise_persistent[sets=2]+", "k_pairwise_persistent[sets=1]+"
COPY1, COPY2 = "k_pairwise_persistent[sets=1]+k_copy_features+", "k_pairwise_persistent[sets=2]+k_copy_features+"
VEC, VEC_COPY = "k_sqnorm<true>+k_pairwise<1>+", "k_sqnorm<true>+k_pairwise<1>[copy]+"
GEN, GEN_COPY = "k_sqnorm<false>+k_pairwise<0>+", "k_sqnorm<false>+k_pairwise<0>[copy]+"
GATHER, CONCAT = "k_gather_anchor_rows+", "pope_concat+"

# n = 257: a ragged last tile for the 32-row and for the 64-row tile.  k = 257: a second column group of the persistent kernel and a
# third of the one-tile kernel, each with one live column; k = 260 (n = 289, ragged for both tiles too): the same with four, next to a
# feature copy in 16-byte pieces.
CASES = {
    # (n, d, k, f, has_x, by_id, knob)
    # the persistent kernel: two sets without x, one beside the side copy; anchors by id are read through the ids (no gather)
    (257, 128, 256, 0, 0, 0, 0): SETS2 + FINISH4,
    (257, 128, 256, 8, 1, 0, 0): COPY1 + FINISH4,
    (257, 128, 256, 8, 1, 1, 0): COPY1 + FINISH4,
    (289, 128, 260, 8, 1, 1, 0): COPY1 + FINISH4,
    (257, 128, 257, 0, 0, 1, 0): SETS2 + FINISH1,
    (257, 36, 257, 0, 0, 0, 0): SETS2 + FINISH1,
    (289, 36, 260, 8, 1, 0, 0): COPY1 + FINISH4,
    (33, 4, 5, 0, 0, 1, 0): SETS2 + FINISH1,
    (257, 128, 256, 0, 1, 0, 0): SETS2 + FINISH4,                       # f = 0: no x, whatever the caller passed
    (257, 128, 256, 8, 0, 0, 0): SETS2 + FINISH4,                       # embedding columns at c0 = 8 of a wider matrix, no x
    # knob 2 / 3: the set count forced, with and without x
    (257, 128, 256, 0, 0, 0, 2): SETS1 + FINISH4,
    (257, 128, 256, 8, 1, 0, 2): COPY1 + FINISH4,
    (257, 128, 256, 0, 0, 0, 3): SETS2 + FINISH4,
    (257, 128, 256, 8, 1, 1, 3): COPY2 + FINISH4,
    # knob 1: the one-tile kernel at a depth the persistent kernel takes; by id: the gather in front
    (257, 128, 256, 8, 1, 0, 1): VEC_COPY + FOLD4,
    (257, 128, 256, 8, 1, 1, 1): GATHER + VEC_COPY + FOLD4,
    (257, 128, 257, 0, 0, 1, 1): GATHER + VEC + FOLD1,
    # depths the persistent kernel does not take
    (257, 132, 256, 8, 1, 0, 0): VEC_COPY + FOLD4,
    (257, 132, 257, 0, 0, 1, 0): GATHER + VEC + FOLD1,
    (257, 7, 257, 0, 0, 0, 0): GEN + FOLD1,
    (257, 7, 256, 8, 1, 1, 0): GATHER + GEN_COPY + FOLD4,
    (257, 130, 256, 8, 1, 0, 0): GEN_COPY + FOLD4,
    (257, 132, 256, 8, 1, 0, 2): VEC_COPY + FOLD4,                      # knobs 2 / 3 choose sets, not the pipeline
    # the feature copy as a pass of its own: f % 4 != 0; (f + k) % 4 != 0
    (257, 128, 256, 6, 1, 0, 0): CONCAT + SETS2 + FINISH1,
    (257, 128, 257, 8, 1, 1, 0): CONCAT + SETS2 + FINISH1,
    (257, 132, 256, 6, 1, 1, 0): CONCAT + GATHER + VEC + FOLD1,
    (257, 7, 257, 8, 1, 0, 0): CONCAT + GEN + FOLD1,
    # rows wider than the side copy takes (16 pieces per lane): pope_concat beside the persistent kernel, inside the one-tile kernel
    (257, 128, 256, 4096, 1, 0, 0): COPY1 + FINISH4,
    (257, 128, 256, 4100, 1, 0, 0): CONCAT + SETS2 + FINISH4,
    (257, 132, 256, 4100, 1, 0, 0): VEC_COPY + FOLD4,
    (257, 128, 256, 4100, 1, 1, 1): GATHER + VEC_COPY + FOLD4,
    # the scaling pass: four columns per lane or one
    (257, 128, 255, 0, 0, 0, 0): SETS2 + FINISH1,
    (257, 132, 255, 0, 0, 0, 0): VEC + FOLD1,
    # n * out_cols * 4 just below and just at 2^32: the persistent kernel's 32-bit store offsets end there
    (4194303, 128, 256, 0, 0, 0, 0): SETS2 + FINISH4,
    (4194304, 128, 256, 0, 0, 0, 0): VEC + FOLD4,
    (1048575, 128, 256, 768, 1, 1, 0): COPY1 + FINISH4,
    (1048576, 128, 256, 768, 1, 1, 0): GATHER + VEC_COPY + FOLD4,
    # the benchmark's call (configs[2])
    (89250, 128, 256, 500, 1, 1, 0): COPY1 + FINISH4,
}

# (N, K, D) of the scratch size queries: N at the edges of the 32-row and 64-row tiles and where 2 * min(ceil(N / 32), 1024) and
# ceil(N / 64) swap order (N = 131072: both 2048); K around the 128-column padding; D = 0: the by-id query answers 0
SCRATCH_SHAPES = [(n, k, d) for n in (1, 31, 32, 33, 64, 65, 257, 89250, 131072, 131073, 200000) for k in (1, 127, 128, 129, 256, 257)
                  for d in (4, 128)] + [(257, 256, 0), (89250, 256, 0), (0, 256, 128), (257, 0, 128)]


@functools.lru_cache(maxsize=None)
def inputs(n, d, k):
    """A zero-mean table with one coincident row pair (rows 5 and 7), and k anchor ids among its rows with row 5 among them: column 0
    holds an anchor's own row (5) and a different row with the same contents (7), both through the cancellation fix-up.  Read-only."""
    emb = pc.offset_table(n, d, 0.0, 1000 * d + k)
    emb[7] = emb[5]
    anchors = pc.anchor_ids(n, k, 1000 * d + k)
    anchors[0] = 5
    emb.setflags(write=False)
    anchors.setflags(write=False)
    return emb, anchors


@functools.lru_cache(maxsize=None)
def want64(n, d, k, fn):
    """scale64(ref64) of inputs(n, d, k): computed once, shared, read-only."""
    emb, anchors = inputs(n, d, k)
    w = pc.scale64(pc.ref64(emb, anchors, fn))
    w.setflags(write=False)
    return w
