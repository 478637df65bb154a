"""The device select over (score, node) pairs behind the five score-ranked sampling methods (utils.py:29-30 and the same two lines
of every method: ascending stable sort, last K), the parts that need no GPU: the order-preserving key of a float64 score, the
argument checks and the scratch query of pope_topk_f64, and the score families and host expression the GPU tests use."""
import ctypes

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("pope_topk_f64", "pope_topk_f64_scratch_bytes", "pope_score_keys_host")
SELECT_N = (1, 2, 63, 64, 65, 256, 257, 1000, 4097, 1024 * 256 + 77)     # the last: TOPK_GRID_CAP * TOPK_BLOCK + 77
SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 5e-324, -5e-324, 0.25, 0.5], dtype=np.float64)
NAN_BITS = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000123],
                    dtype=np.uint64)                                     # quiet, negative, signalling, all ones, a payload


@pytest.fixture(autouse=True)
def _clean_error_string():
    """The library's error string is per thread and outlives a test; a successful host-only call clears it."""
    yield
    from graphpope_amd import _lib
    buf = ctypes.create_string_buffer(64)
    _lib.check(_lib.load().pope_level_kernel_name(89250, 256, buf, 64))
    assert _lib.load().pope_last_error() == b""


# ------------------------------------------------------------------------------------------------ shared with the GPU tests
def host_line(scores, k):
    """The line the select replaces: np.argsort(score, kind="stable")[-k:]."""
    return np.argsort(scores, kind="stable")[-k:]


def select_ks(n, cap):
    return sorted({k for k in (1, 2, min(n, 64), n - 1, n, cap) if 1 <= k <= min(n, cap)})


def score_keys(x):
    from graphpope_amd import _lib
    x = np.ascontiguousarray(x, dtype=np.float64)
    keys = np.zeros(x.shape[0], dtype=np.uint64)
    _lib.check(_lib.load().pope_score_keys_host(x.ctypes.data_as(ctypes.c_void_p), x.shape[0], keys.ctypes.data_as(ctypes.c_void_p)))
    return keys


def score_families(n, seed=0):
    """(name, float64 [n]) for the select tests."""
    rs = np.random.RandomState(seed + 17 * n)
    ids = np.arange(n, dtype=np.float64)
    yield "all_equal", np.full(n, 0.375)
    for name, lower in (("two_values_mostly_upper", n // 4), ("two_values_mostly_lower", n - n // 4), ("two_values_halves", n // 2)):
        x = np.ones(n)                                                   # with K in {1, 2, 64, N - 1, N, cap} the K-th pair falls inside
        x[rs.permutation(n)[:lower]] = 0.0                               # the upper class, inside the lower one, and (below) on the boundary
        yield name, x
    x = np.zeros(n)
    x[n - min(n, 64):] = 1.0                                             # exactly min(N, 64) in the upper class: K = min(N, 64) cuts at the boundary
    yield "two_values_boundary_at_64", x[::-1].copy()                    # ... which sits at the low ids
    x = rs.rand(n) * 0.5                                                 # a tie class ABOVE everything else whose members sit astride
    tie = [i for i in (62, 63, 64, 65, 254, 255, 256, 257) if i < n]     # wave and block edges: K = 1, 2 cut it
    x[tie] = 0.75
    yield "tie_class_on_wave_and_block_edges", x
    x = rs.rand(n) + 1.0
    x[tie] = 0.5                                                         # the same class BELOW everything else: K = N - 1 cuts it
    yield "tie_class_at_the_bottom", x
    yield "all_distinct", rs.permutation(n).astype(np.float64) * 1.25 - n / 3.0
    yield "lowest_mantissa_bit", (np.uint64(0x3FE5555555555554) | rs.randint(0, 2, n).astype(np.uint64)).view(np.float64)
    yield "top_byte_only", ((rs.randint(0, 256, n).astype(np.uint64) << np.uint64(56)) | np.uint64(0x000FEDCBA9876543)).view(np.float64)
    yield "negatives_and_zeros", rs.choice(np.array([-2.5, -1.0, -0.0, 0.0, -5e-324, -0.125]), n)
    x = rs.choice(np.array([np.inf, -np.inf, 0.0, 1.0, -1.0, 3.5]), n)
    nan = rs.rand(n) < 0.3
    x[nan] = rs.choice(NAN_BITS, int(nan.sum())).view(np.float64)
    yield "nan_and_inf", x
    yield "denormals", (rs.randint(0, 8, n).astype(np.uint64) | (rs.randint(0, 2, n).astype(np.uint64) << np.uint64(63))).view(np.float64)
    yield "score_is_node_id", ids.copy()
    yield "score_is_minus_node_id", -ids


# ------------------------------------------------------------------------------------------------ tests
def test_symbols_are_exported_and_declared():
    from graphpope_amd import _lib
    lib = _lib.load()
    header = open(ROOT + "/include/graphpope_hip.h").read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name


def _bits_to_float(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def test_key_transform_orders_as_numpy_sorts():
    """np.lexsort((arange, keys)) == np.argsort(x, kind="stable") on vectors drawn from +-0.0, +-1.0, +-inf, NaNs with different
    payloads and signs, +-5e-324, 0.25 and 0.5: unsigned comparison of the keys, ties by index, IS NumPy's stable order."""
    pool = np.concatenate([SPECIALS, _bits_to_float(NAN_BITS)])
    rs = np.random.RandomState(7)
    for n in (1, 2, 15, 64, 1000):
        for _ in range(8):
            x = pool[rs.randint(0, len(pool), n)]
            keys = score_keys(x)
            assert np.array_equal(np.lexsort((np.arange(n), keys)), np.argsort(x, kind="stable")), x
    x = pool.copy()
    keys = score_keys(x)
    assert np.array_equal(np.lexsort((np.arange(len(x)), keys)), np.argsort(x, kind="stable"))


def test_key_transform_values():
    k = score_keys(np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf]), _bits_to_float(NAN_BITS)]))
    assert k[0] == k[1] == np.uint64(0x8000000000000000)                 # -0.0 is +0.0
    assert k[2] == np.uint64(0xBFF0000000000000) and k[3] == np.uint64(0x400FFFFFFFFFFFFF)
    assert k[4] == np.uint64(0xFFF0000000000000) and k[5] == np.uint64(0x000FFFFFFFFFFFFF)
    assert (k[6:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()                # every NaN, above +inf
    rs = np.random.RandomState(3)
    x = (rs.randint(1, 1 << 61, 4000).astype(np.uint64) << np.uint64(2)).view(np.float64)      # positive: bit 63 clear
    x = np.unique(x[np.isfinite(x)])
    k = score_keys(np.concatenate([-x[::-1], x]))
    assert (np.diff(k.astype(object)) > 0).all()                         # strictly monotone over ordinary values of both signs


def test_key_helper_validates():
    from graphpope_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 4)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    assert lib.pope_score_keys_host(null, 4, p) == _lib.ERR_INVALID and b"pope_score_keys_host" in lib.pope_last_error()
    assert lib.pope_score_keys_host(p, 4, null) == _lib.ERR_INVALID
    assert lib.pope_score_keys_host(p, -1, p) == _lib.ERR_INVALID
    assert lib.pope_score_keys_host(null, 0, null) == _lib.OK


def test_scratch_query_needs_no_gpu():
    from graphpope_amd import _lib
    lib = _lib.load()
    q, cap = lib.pope_topk_f64_scratch_bytes, lib.pope_topk_max_k()
    flickr = q(89250, 256)
    assert flickr >= 2 * 89250 * 12 + 256 * 12 + 12 * 256 * 4            # two pair buffers, K pairs, twelve histograms
    assert q(2 * 89250, 256) > flickr and q(1 << 22, 512) > q(2 * 89250, 256)
    assert q(89250, 257) >= flickr
    assert q(0, 1) == 0 and q(-5, 1) == 0 and q((1 << 31) - 1, 1) == 0 and q(1 << 31, 1) == 0
    assert q(100, 0) == 0 and q(100, -1) == 0
    assert q(100, 101) == 0                                              # K > N
    assert q(1 << 20, cap + 1) == 0 and q(1 << 20, cap) > 0              # K > cap
    assert q(1, 1) > 0
    assert lib.pope_last_error() == b""


def test_argument_validation_needs_no_gpu():
    """Null pointers, N and K out of range and a short scratch are refused before any HIP call, with the entry's name in the
    message; scores_out alone may be null."""
    from graphpope_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def topk(scores=p, n=1000, k=10, nodes=p, scores_out=p, scratch=p, scratch_bytes=1 << 30):
        return lib.pope_topk_f64(scores, n, k, nodes, scores_out, scratch, scratch_bytes, null)

    for kw in ("scores", "nodes", "scratch"):
        assert topk(**{kw: null}) == _lib.ERR_INVALID, kw
        assert b"pope_topk_f64" in lib.pope_last_error() and b"null pointer" in lib.pope_last_error()
    for n in (0, -1, (1 << 31) - 1, 1 << 31):
        assert topk(n=n, k=1) == _lib.ERR_INVALID, n
        assert lib.pope_last_error().startswith(b"pope_topk_f64")
    cap = lib.pope_topk_max_k()
    for n, k in ((1000, 0), (1000, -3), (1000, 1001), (1 << 20, cap + 1)):
        assert topk(n=n, k=k) == _lib.ERR_INVALID, (n, k)
        assert lib.pope_last_error().startswith(b"pope_topk_f64") and b"K" in lib.pope_last_error()
    need = lib.pope_topk_f64_scratch_bytes(1000, 10)
    for short in (need - 1, 0):
        assert topk(scratch_bytes=short) == _lib.ERR_WORKSPACE
        assert lib.pope_last_error().startswith(b"pope_topk_f64") and b"scratch" in lib.pope_last_error()
        assert topk(scratch_bytes=short, scores_out=null) == _lib.ERR_WORKSPACE     # a null scores_out is no error of its own


def test_engine_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from graphpope_amd import engine
    x = np.arange(5, dtype=np.float64)
    for k in (2, 0, 9):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            engine.score_anchors(x, k)


def test_engine_wants_a_float64_vector():
    from graphpope_amd import engine
    for bad in (np.arange(5, dtype=np.float32), np.zeros((2, 3)), np.arange(5)):
        with pytest.raises(ValueError, match="float64 vector"):
            engine.score_anchors(bad, 2)


def test_score_families_are_what_they_claim():
    n = 4097
    fam = dict(score_families(n))
    assert len(fam) == 15 and all(v.dtype == np.float64 and v.shape == (n,) for v in fam.values())
    assert len(np.unique(fam["all_equal"])) == 1 and len(np.unique(fam["all_distinct"])) == n
    for name in ("two_values_mostly_upper", "two_values_mostly_lower", "two_values_halves", "two_values_boundary_at_64"):
        assert set(np.unique(fam[name]).tolist()) == {0.0, 1.0}
    upper = {name: int(fam[name].sum()) for name in fam if name.startswith("two_values")}
    assert upper["two_values_mostly_upper"] > 64 > 2                     # K = 1, 2, 64: inside the upper class
    assert n - 1 > upper["two_values_mostly_lower"] and upper["two_values_mostly_lower"] < 4096   # K = cap, N - 1: inside the lower class
    assert upper["two_values_boundary_at_64"] == 64                      # K = 64: the whole upper class and nothing else
    assert (fam["two_values_boundary_at_64"][:64] == 1.0).all()
    t = fam["tie_class_on_wave_and_block_edges"]
    assert np.flatnonzero(t == t.max()).tolist() == [62, 63, 64, 65, 254, 255, 256, 257]
    b = fam["tie_class_at_the_bottom"]
    assert np.flatnonzero(b == b.min()).tolist() == [62, 63, 64, 65, 254, 255, 256, 257]
    bits = fam["lowest_mantissa_bit"].view(np.uint64)
    assert set(np.unique(bits ^ bits.min()).tolist()) == {0, 1}
    bits = fam["top_byte_only"].view(np.uint64)
    assert ((bits ^ bits[0]) & np.uint64(0x00FFFFFFFFFFFFFF) == 0).all() and len(np.unique(bits)) > 200
    z = fam["negatives_and_zeros"]
    assert (z <= 0).all() and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    s = fam["nan_and_inf"]
    assert np.isnan(s).any() and np.isposinf(s).any() and np.isneginf(s).any() and len(np.unique(s[np.isnan(s)].view(np.uint64))) > 1
    d = fam["denormals"]
    assert (np.abs(d) < 2.3e-308).all() and (d < 0).any() and (d > 0).any()
    assert np.array_equal(fam["score_is_node_id"], -fam["score_is_minus_node_id"])


@pytest.mark.parametrize("n", SELECT_N[:-1])
def test_keys_and_node_ids_restate_the_host_line(n):
    """What the kernel selects -- the K largest (key, node) pairs, ascending -- is the host line on every family."""
    for name, x in score_families(n):
        order = np.lexsort((np.arange(n), score_keys(x)))
        want = np.argsort(x, kind="stable")
        assert np.array_equal(order, want), name
        for k in select_ks(n, 4096):
            assert np.array_equal(order[-k:], host_line(x, k)), (name, k)
