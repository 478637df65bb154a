"""Shared by tests/test_node2vec_loss_cpu.py and tests/test_node2vec_loss_gpu.py.  Not a test module.

1. ``reference``: the contract of pope_n2v_loss_grad (include/graphpope_hip.h) restated in NumPy float64, straight from walk rows
   [R, len] -- no window matrix, no autograd -- together with the same expressions on absolute values (the magnitudes the error
   bounds are relative to, in the style of sage_backward_cases.Reference.magnitude).
2. The bounds, derived from the kernels' arithmetic and not from what they return (u = 2^-24, float32's unit roundoff):

   contrib[r, i, d] (pope_n2v_position_grads)   (2 (C - 1) + 2) u A[r, i, d]
       A position takes part in t <= 2 (C - 1) pairs: as the start of its own window and as a context of up to C - 1 earlier ones.
       Its row is sum_t coef_t e_t[d]: the float64 coefficient rounded once to float32 (one u per term), then a float32 dot product
       of t terms accumulated one after the other -- within t u of the exact sum, relative to sum |coef_t| |e_t[d]| = A, to first
       order and whether or not a product is fused into its addition.  (t + 1) u A; one more u A of slack takes the higher-order
       terms and the float64 arithmetic in front (products, exp, log: 1e-16 relative against u = 6e-8).
   grad[v, d], atomic form (pope_n2v_loss_grad)  (2 (C - 1) + n_v + 3) u sum_{positions of v} A
       The n_v rows of the positions that hold v come together through at most n_v float32 additions, in any order: a wave's first
       row of v is STORED to its LDS slot, every later one added there, the slot leaves as one atomic add; without a slot a row is
       one atomic add.  Every row passes through at most n_v additions: n_v u more, relative to the same magnitude.
   grad[v, d], deterministic form (position_grads + accumulate_det)   sum of the position bounds + u |want|
       The rows are added in float64 (exact to 1e-16) and the sum is rounded to float32 once.
   loss                                          (T + 64) 2^-53 scale sum |term|,  T terms
       Float64 throughout: a sum of T terms in any order is within (T - 1) 2^-53 of the exact one relative to sum |term|; the 64
       take the few units every term carries itself (the product summed in another order, exp, log).  T < 8000 keeps it under 1e-12.

3. The inputs: embedding rows randn * 2 / sqrt(D) (products of order 1; ``reference`` reports the largest |out|, the tests assert
   it below 6, where neither literal form -log(sigmoid + 1e-15) / -log(1 - sigmoid + 1e-15) cancels), and row ids from three
   populations (POPULATIONS).
4. The case table (CASES), the largest row lengths the two LDS formulas of the header accept, and the scan case of
   pope_n2v_accumulate_det.
5. SparseAdam: the documented update as NumPy float32 operations, each rounded once (``sparse_adam_reference``).
"""
import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import node2vec_det_cases as det_cases

U = 2.0 ** -24
EPS = 1e-15
ROWS_PER_WAVE, SLOTS = 8, 16                      # N2V_ROWS_PER_WAVE, N2V_SLOTS of csrc/node2vec.hip
LDS_LIMIT = 65536
OUT_LIMIT = 6.0
MAX_TERMS = 8000


# ---- the header's LDS formulas -------------------------------------------------------------------------------------------------
def loss_grad_lds_bytes(length, c, d):
    """(len (D + 1) + (len + 1 - context)(context - 1) + 16 D) * 4 + 4 (len + 16)"""
    return (length * (d + 1) + (length + 1 - c) * (c - 1) + SLOTS * d) * 4 + 4 * (length + SLOTS)


def position_grads_lds_bytes(length, c, d):
    """(len (D + 1) + (len + 1 - context)(context - 1)) * 4 + 4 (len + 16)"""
    return (length * (d + 1) + (length + 1 - c) * (c - 1)) * 4 + 4 * (length + SLOTS)


def largest_len(formula, c, d):
    length = c
    while formula(length + 1, c, d) <= LDS_LIMIT:
        length += 1
    assert formula(length, c, d) <= LDS_LIMIT
    return length


LDS_C, LDS_D = 2, 256
LDS_LEN_LOSS_GRAD = largest_len(loss_grad_lds_bytes, LDS_C, LDS_D)
LDS_LEN_POSITION_GRADS = largest_len(position_grads_lds_bytes, LDS_C, LDS_D)
assert (LDS_LEN_LOSS_GRAD, LDS_LEN_POSITION_GRADS) == (47, 63)
assert loss_grad_lds_bytes(47, LDS_C, LDS_D) == 65136 and loss_grad_lds_bytes(48, LDS_C, LDS_D) > LDS_LIMIT


# ---- the case table ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    family: str
    length: int
    c: int
    d: int
    r: int
    forms: str = "both"            # "both", or the one form whose LDS formula accepts the row: "atomic" / "det"
    bad: bool = False              # row 3 holds N and row 5 holds -1

    @property
    def name(self):
        return f"{self.family}-len{self.length}-C{self.c}-D{self.d}-R{self.r}"

    @property
    def pairs(self):               # P: the (window, context slot) pairs of one row
        return (self.length + 1 - self.c) * (self.c - 1)


CASES = (
    [Case("reference-shape", 21, 10, 128, 17), Case("P64", 16, 9, 32, 9), Case("P65", 18, 6, 32, 9)]
    + [Case("ids-rounds", length, 2, 32, 3) for length in (64, 65, 130)]
    + [Case("window-form", length, length, 64, 9) for length in (2, 21)]
    + [Case("width", 9, 4, d, 8) for d in (32, 64, 96, 160, 192, 224, 256)]
    + [Case("rows-per-wave", 8, 4, 32, r) for r in (1, 7, 8, 9)]
    + [Case("largest-lds", LDS_LEN_LOSS_GRAD, LDS_C, LDS_D, 2, forms="atomic"),
       Case("largest-lds", LDS_LEN_POSITION_GRADS, LDS_C, LDS_D, 2, forms="det")]
    + [Case("bad-rows", 8, 4, 32, 9, bad=True)]
)
ATOMIC_CASES = [c for c in CASES if c.forms in ("both", "atomic")]
DET_CASES = [c for c in CASES if c.forms in ("both", "det")]
assert CASES[0].pairs == 108 and CASES[1].pairs == 64 and CASES[2].pairs == 65
assert all(c.pairs == c.length - 1 for c in CASES if c.family == "ids-rounds")

# The populations the row ids are drawn from.  3: every wave merges long chains into few LDS slots, n_v is large.  40: the 8 rows of
# a wave meet more than 16 distinct nodes and repeat some -- slot path and straight-to-memory path.  5000, all ids of a call
# distinct: nothing merges and the slots run out at the 17th node.
POPULATIONS = (3, 40, 5000)
NEGATIVE = (0, 1)


@lru_cache(maxsize=None)
def table(n, d):
    """float32 [n, d], rows randn * 2 / sqrt(d): a pure function of (n, d).  In the small populations a node is often its own context,
    so |e|^2 (4 on average, +-1 at d = 32) is a product too: a row with |e|^2 >= 5.5 is drawn again, which keeps every |out| < 6."""
    rng = np.random.default_rng(1000 * d + n)
    t = (rng.standard_normal((n, d)) * (2.0 / math.sqrt(d))).astype(np.float32)
    for _ in range(100):
        again = np.nonzero((t.astype(np.float64) ** 2).sum(axis=1) >= 5.5)[0]
        if not len(again):
            break
        t[again] = (rng.standard_normal((len(again), d)) * (2.0 / math.sqrt(d))).astype(np.float32)
    assert not len(again)
    t.setflags(write=False)
    return t


@lru_cache(maxsize=None)
def walk_rows(case, n):
    """int64 [R, len] from population n; 5000: all ids distinct.  The bad case: row 3 holds n, row 5 holds -1."""
    rng = np.random.default_rng([case.length, case.c, case.d, case.r, n])
    size = case.r * case.length
    ids = rng.permutation(n)[:size] if n == 5000 else rng.integers(0, n, size=size)
    assert len(ids) == size
    rows = ids.reshape(case.r, case.length).astype(np.int64)
    if case.bad:
        rows[3, 5], rows[5, 0] = n, -1
    rows.setflags(write=False)
    return rows


def scale_of(case):
    """1 / (the number of terms of the call, bad rows counted: the scale a caller forms from the shape)."""
    return 1.0 / (case.r * case.pairs)


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------
class Result:
    """pos_grad [R, len, D] and its magnitude A; nodes [K]: the ids that occur in valid rows, ascending; grad [K, D] (the gradient rows
    of ``nodes``: every other row of the gradient is zero) and its magnitude grad_mag; n_v [K]; loss (scaled); row_loss [R] (unscaled)
    and row_abs [R] (sum |term|); terms (T, of the valid rows); max_out; valid [R]."""


def reference(emb, rows, c, negative, scale):
    """The contract of pope_n2v_loss_grad on walk rows.  Per pair (j, k), 1 <= k < c, of a row whose ids all lie in [0, N):
    out = <e_j, e_{j + k}>, term = -log(sigmoid(out) + 1e-15) or -log(1 - sigmoid(out) + 1e-15), coef = scale * d term / d out;
    pos_grad[j] += coef e_{j + k}, pos_grad[j + k] += coef e_j.  The products of two float32 values are exact in float64 and are
    added in extended precision where the platform has it, so `out` carries one rounding."""
    n, d = emb.shape
    r_count, length = rows.shape
    w = length + 1 - c
    e64 = emb.astype(np.float64)
    res = Result()
    res.pos_grad = np.zeros((r_count, length, d))
    res.A = np.zeros((r_count, length, d))
    res.row_loss, res.row_abs = np.zeros(r_count), np.zeros(r_count)
    res.valid = ((rows >= 0) & (rows < n)).all(axis=1)
    res.max_out = 0.0
    for r in np.nonzero(res.valid)[0]:
        e = e64[rows[r]]
        for k in range(1, c):
            a, b = e[0:w], e[k:k + w]
            out = (a * b).astype(np.longdouble).sum(axis=1).astype(np.float64)
            sg = 1.0 / (1.0 + np.exp(-out))
            q = ((1.0 - sg) if negative else sg) + EPS
            term = -np.log(q)
            dq = sg * (1.0 - sg)
            coef = scale * (dq if negative else -dq) / q
            res.pos_grad[r, 0:w] += coef[:, None] * b
            res.pos_grad[r, k:k + w] += coef[:, None] * a
            res.A[r, 0:w] += np.abs(coef)[:, None] * np.abs(b)
            res.A[r, k:k + w] += np.abs(coef)[:, None] * np.abs(a)
            res.row_loss[r] += term.sum()
            res.row_abs[r] += np.abs(term).sum()
            res.max_out = max(res.max_out, float(np.abs(out).max()))
    res.terms = int(res.valid.sum()) * w * (c - 1)
    res.loss = scale * float(res.row_loss.sum())
    flat = rows[res.valid].reshape(-1)
    res.nodes, where = np.unique(flat, return_inverse=True)
    res.grad, res.grad_mag = np.zeros((len(res.nodes), d)), np.zeros((len(res.nodes), d))
    np.add.at(res.grad, where, res.pos_grad[res.valid].reshape(-1, d))
    np.add.at(res.grad_mag, where, res.A[res.valid].reshape(-1, d))
    res.n_v = np.bincount(where, minlength=len(res.nodes))
    res.c, res.scale, res.pairs = c, scale, w * (c - 1)
    return res


def bounds(res):
    """dict: contrib [R, len, D], grad_atomic [K, D], grad_det [K, D], loss (scalar), row_loss [R].  See the module docstring."""
    cm = res.c - 1
    contrib = (2 * cm + 2) * U * res.A
    return {
        "contrib": contrib,
        "grad_atomic": (2 * cm + res.n_v[:, None] + 3) * U * res.grad_mag,
        "grad_det": (2 * cm + 2) * U * res.grad_mag + U * np.abs(res.grad),      # the sum of the position bounds, plus u |want|
        "loss": (res.terms + 64) * 2.0 ** -53 * res.scale * float(res.row_abs.sum()),
        "row_loss": (res.pairs + 64) * 2.0 ** -53 * res.row_abs,                 # unscaled, T = the P terms of one row
    }


@lru_cache(maxsize=None)
def solved(case, n, negative):
    """(emb, rows, scale, reference, bounds) of one run: computed once, shared by the tests, never written to."""
    emb, rows, scale = table(n, case.d), walk_rows(case, n), scale_of(case)
    res = reference(emb, rows, case.c, negative, scale)
    return emb, rows, scale, res, bounds(res)


# ---- the scan of pope_n2v_accumulate_det ---------------------------------------------------------------------------------------
SCAN_D, SCAN_M = 32, 3000
SCAN_N = (512, 513, 8192, 8193, 20000)       # one wave of the scan exactly / one node more; one round of 8192 exactly / one more; 3 rounds
SCAN_EDGES = (0, 511, 512, 8191, 8192)       # and N - 1: the first and last node of a scan wave and of a scan round
SCAN_LONG = 100                              # a list longer than a wave, past the first round where N allows


def scan_ids(n, rng):
    """int32 [SCAN_M], shuffled: 3 entries on each of the nodes 0, 511, 512, 8191, 8192, N - 1 that exist, SCAN_LONG entries on node
    9000 (N > 9000; else on node 300), 10 entries each of -1 and N, and the rest on 150 other nodes spread over [0, N)."""
    edges = sorted({v for v in SCAN_EDGES + (n - 1,) if v < n})
    long_node = 9000 if n > 9000 else 300
    fixed = [v for v in edges for _ in range(3)] + [long_node] * SCAN_LONG + [-1] * 10 + [n] * 10
    others = np.setdiff1d(rng.choice(n, size=min(n, 400), replace=False), np.array(edges + [long_node]))[:150]
    ids = np.concatenate([np.array(fixed), rng.choice(others, size=SCAN_M - len(fixed))]).astype(np.int32)
    rng.shuffle(ids)
    count = np.bincount(ids[(ids >= 0) & (ids < n)], minlength=n)
    assert len(ids) == SCAN_M and all(count[v] == 3 for v in edges) and count[long_node] == SCAN_LONG
    assert (count == 0).sum() >= n - 160 and count.max() <= SCAN_LONG
    return ids


@lru_cache(maxsize=None)
def scan_case(n):
    """(ids [M], contrib [M, D] with cancellation lists, prior grad [N, D], the reference's grad, its touched)."""
    rng = np.random.default_rng(n)
    ids = scan_ids(n, rng)
    contrib = det_cases.cancellation_lists(ids, n, SCAN_D, rng)
    prior = rng.standard_normal((n, SCAN_D)).astype(np.float32)
    want, touched = det_cases.accumulate_reference(ids, contrib, prior)
    return ids, contrib, prior, want, touched


# ---- SparseAdam ----------------------------------------------------------------------------------------------------------------
def sparse_adam_scalars(lr, beta1, beta2, eps, step):
    """(-step_size, 1 - beta1, 1 - beta2, eps) as float32: formed in double and rounded once, as the launcher forms them."""
    bc1, bc2 = 1.0 - math.pow(beta1, float(step)), 1.0 - math.pow(beta2, float(step))
    return np.float32(-(lr * math.sqrt(bc2) / bc1)), np.float32(1.0 - beta1), np.float32(1.0 - beta2), np.float32(eps)


def sparse_adam_reference(p, m, v, g, flagged, lr, beta1, beta2, eps, step):
    """(p, m, v) after one step on the rows in ``flagged``; the other rows are returned as they came.  NumPy float32 operations, each
    rounded once to nearest:  m += (g - m)(1 - b1);  v += (g g - v)(1 - b2);  p += -step_size * (m / (sqrt(v) + eps))."""
    neg_step, omb1, omb2, eps32 = sparse_adam_scalars(lr, beta1, beta2, eps, step)
    p, m, v = p.copy(), m.copy(), v.copy()
    for a in (p, m, v, g):
        assert a.dtype == np.float32
    f = np.asarray(flagged, dtype=np.int64)
    gf = g[f]
    mn = m[f] + (gf - m[f]) * omb1
    vn = v[f] + (gf * gf - v[f]) * omb2
    upd = mn / (np.sqrt(vn) + eps32)
    pn = p[f] + neg_step * upd
    for a in (mn, vn, upd, pn):
        assert a.dtype == np.float32
    p[f], m[f], v[f] = pn, mn, vn
    return p, m, v


ADAM_LR, ADAM_BETAS, ADAM_EPS = 0.01, (0.9, 0.999), 1e-8
ADAM_GRID_CAP = 2048 * 64                    # rows one pass of the launch covers (2 048 blocks of 64 flags): past it a block takes a second group
ADAM_SHAPES = [(n, 32) for n in (1, 63, 64, 65, 129, 1000)] + [(129, d) for d in (96, 160, 256)] + [(ADAM_GRID_CAP + 65, 32)]


def sparse_adam_steps(n, d):
    """Three steps [(flagged rows, gradient rows [len(flagged), d])]: rows 0, 63, 64 and n - 1 where they exist plus a random third of
    the others; the elements of a step's gradient span 1e-3 .. 1e3 (per row 10^uniform(-3, 3)); the last step flags nothing."""
    rng = np.random.default_rng(100 * n + d)
    steps = []
    for _ in range(2):
        rows = sorted({v for v in (0, 63, 64, n - 1) if v < n} | set(np.nonzero(rng.random(n) < 1 / 3)[0].tolist()))
        scale = 10.0 ** rng.uniform(-3, 3, size=(len(rows), 1))
        scale[:2, 0] = (1e-3, 1e3)[:len(rows)]
        steps.append((np.array(rows, dtype=np.int64), (rng.standard_normal((len(rows), d)) * scale).astype(np.float32)))
    steps.append((np.zeros(0, dtype=np.int64), np.zeros((0, d), dtype=np.float32)))
    return steps
