"""Degree-centrality anchors (utils.py:38-42 nx.degree_centrality, ascending stable sort, last K), the parts that need no GPU:
the four C-ABI symbols, their argument checks and the scratch query, the engine's refusal to run without a device, the host
formula the GPU tests compare with, and a NumPy restatement of the radix select that pins the algorithm of pope_topk_u64."""
import ctypes

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("pope_degree_counts", "pope_topk_scratch_bytes", "pope_topk_u64", "pope_topk_max_k")
SELECT_N = (1, 63, 64, 65, 257, 4097, 100003)


@pytest.fixture(autouse=True)
def _clean_error_string():
    """The library's error string is per thread and outlives a test: the rejected calls below would leave theirs to whichever
    test runs next in this process (test_abi reads it as empty).  A successful host-only call clears it."""
    yield
    from graphpope_amd import _lib
    buf = ctypes.create_string_buffer(64)
    _lib.check(_lib.load().pope_level_kernel_name(89250, 256, buf, 64))
    assert _lib.load().pope_last_error() == b""


# ------------------------------------------------------------------------------------------------ shared with the GPU tests
def host_degrees(ei, n):
    """In + out degree over the distinct (u, v) pairs: the expression of sample_anchor_nodes' host branch."""
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    pairs = np.unique(ei[0] * n + ei[1])
    return np.bincount(pairs // n, minlength=n) + np.bincount(pairs % n, minlength=n)


def host_anchors(ei, n, k):
    """The list sample_anchor_nodes(..., 'degree_centrality') returns on a machine without a GPU."""
    return np.argsort(host_degrees(ei, n), kind="stable")[-k:].tolist()


def digraph(ei, n):
    import networkx as nx
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    ei = np.asarray(ei).reshape(2, -1)
    g.add_edges_from(zip(ei[0].tolist(), ei[1].tolist()))
    return g


def cli_graph():
    """The graph of test_cli.py's degree test: directed R-MAT 8 with repeated edges and self-loops."""
    from graphpope_amd import synth
    ei, n = synth.rmat(8, edge_factor=4, seed=3, symmetric=False)
    return np.concatenate([ei, ei[:, :50], np.stack([np.arange(5), np.arange(5)])], axis=1), n


def select_ks(n, cap):
    return sorted({1, min(n, 2), min(n, 64), min(n, cap)})


def key_sets(n, k, seed=0):
    """(name, uint64 [n]) for the select tests: all equal; distinct over the full 64 bits, half with bit 63 set; keys that
    differ in exactly one of the eight bytes; exactly k - 1 keys above a value held by 500 duplicates (as many as fit when
    n < k - 1 + 500: the threshold then still lies in the run of ties, or is its only member)."""
    rs = np.random.RandomState(seed + 31 * n + k)
    yield "all_equal", np.full(n, 0x8123456789ABCDEF, dtype=np.uint64)
    low = rs.permutation(n).astype(np.uint64)                            # distinct in the low 20 bits
    rnd = (rs.randint(0, 1 << 21, n).astype(np.uint64) << np.uint64(42)) | (rs.randint(0, 1 << 22, n).astype(np.uint64) << np.uint64(20))
    top = (np.arange(n) % 2).astype(np.uint64) << np.uint64(63)
    yield "distinct_full_range", (top | rnd | low)[rs.permutation(n)]
    for byte in range(8):
        base = np.uint64(0x5A5A5A5A5A5A5A5A) & ~(np.uint64(0xFF) << np.uint64(8 * byte))
        yield f"byte_{byte}", base | (rs.randint(0, 256, n).astype(np.uint64) << np.uint64(8 * byte))
    dup = min(500, n - (k - 1))
    t = np.uint64(0x00000007_00000000)
    above = t + np.uint64(1) + rs.randint(0, 1 << 30, k - 1).astype(np.uint64)
    below = rs.randint(0, 1 << 30, n - dup - (k - 1)).astype(np.uint64)
    keys = np.concatenate([above, np.full(dup, t, dtype=np.uint64), below])
    yield "threshold_in_ties", keys[rs.permutation(n)]


def select_restated(keys, k):
    """The algorithm of pope_topk_u64 in NumPy: eight digits from the most significant one -- histogram of the digit over the
    candidates, the bin that holds the k-th largest, everything above the bin goes to the result, the bin becomes the
    candidates; then the threshold T fills what is left, and the k keys are sorted."""
    cand = np.asarray(keys, dtype=np.uint64)
    remaining, prefix, taken = int(k), 0, []
    for d in range(8):
        shift = np.uint64(56 - 8 * d)
        digit = ((cand >> shift) & np.uint64(0xFF)).astype(np.int64)
        hist = np.bincount(digit, minlength=256)
        above = np.concatenate([np.cumsum(hist[::-1])[::-1][1:], [0]])   # keys in the bins above each bin
        b = int(np.flatnonzero((above < remaining) & (remaining <= above + hist))[0])
        taken.append(cand[digit > b])
        remaining -= int(above[b])
        prefix |= b << int(shift)
        cand = cand[digit == b]
        assert 1 <= remaining <= len(cand)
    assert (cand == np.uint64(prefix)).all()
    out = np.concatenate(taken + [np.full(remaining, prefix, dtype=np.uint64)])
    assert len(out) == k
    return np.sort(out)


# ------------------------------------------------------------------------------------------------ tests
def test_symbols_are_exported_and_declared():
    from graphpope_amd import _lib
    lib = _lib.load()
    header = open(ROOT + "/include/graphpope_hip.h").read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header, name
    assert lib.pope_topk_max_k() >= 1024
    assert f"#define POPE_TOPK_MAX_K {lib.pope_topk_max_k()}\n" in header


def test_scratch_query_needs_no_gpu():
    from graphpope_amd import _lib
    lib = _lib.load()
    q, cap = lib.pope_topk_scratch_bytes, lib.pope_topk_max_k()
    flickr = q(89250, 256)
    assert flickr > 0
    assert q(2 * 89250, 256) > flickr and q(1 << 22, 512) > q(2 * 89250, 256)
    assert q(0, 1) == 0 and q(-5, 1) == 0 and q(1 << 31, 1) == 0
    assert q(100, 0) == 0 and q(100, -1) == 0
    assert q(100, 101) == 0                                              # K > N
    assert q(1 << 20, cap + 1) == 0 and q(1 << 20, cap) > 0              # K > cap
    assert q(1, 1) > 0
    assert lib.pope_last_error() == b""


def test_argument_validation_needs_no_gpu():
    """Null pointers, N and K out of range and a short scratch are refused before any HIP call, with the function's name in the
    message."""
    from graphpope_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def counts(r=p, c=p, er=p, n=8, deg=p, keys=p):
        return lib.pope_degree_counts(r, c, er, n, deg, keys, null)

    for kw in ("r", "c", "er", "deg"):
        assert counts(**{kw: null}) == _lib.ERR_INVALID, kw
        assert b"pope_degree_counts" in lib.pope_last_error() and b"null pointer" in lib.pope_last_error()
    for n in (0, -1, (1 << 31) - 1, 1 << 31):
        assert counts(n=n) == _lib.ERR_INVALID, n
        assert lib.pope_last_error().startswith(b"pope_degree_counts")

    def topk(keys=p, n=1000, k=10, out=p, scratch=p, scratch_bytes=1 << 30):
        return lib.pope_topk_u64(keys, n, k, out, scratch, scratch_bytes, null)

    for kw in ("keys", "out", "scratch"):
        assert topk(**{kw: null}) == _lib.ERR_INVALID, kw
        assert b"pope_topk_u64" in lib.pope_last_error() and b"null pointer" in lib.pope_last_error()
    for n in (0, -1, (1 << 31) - 1, 1 << 31):
        assert topk(n=n, k=1) == _lib.ERR_INVALID, n
        assert lib.pope_last_error().startswith(b"pope_topk_u64")
    cap = lib.pope_topk_max_k()
    for n, k in ((1000, 0), (1000, -3), (1000, 1001), (1 << 20, cap + 1)):
        assert topk(n=n, k=k) == _lib.ERR_INVALID, (n, k)
        assert lib.pope_last_error().startswith(b"pope_topk_u64") and b"K" in lib.pope_last_error()
    need = lib.pope_topk_scratch_bytes(1000, 10)
    assert topk(scratch_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert lib.pope_last_error().startswith(b"pope_topk_u64") and b"scratch" in lib.pope_last_error()
    assert topk(scratch_bytes=0) == _lib.ERR_WORKSPACE


def test_engine_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from graphpope_amd import engine
    ei = torch.as_tensor(np.array([[0, 1], [1, 2]], dtype=np.int64))
    for call in (lambda: engine.degree_counts(ei, 3), lambda: engine.degree_centrality(ei, 3), lambda: engine.degree_centrality(ei, 1),
                 lambda: engine.degree_anchors(ei, 3, 2), lambda: engine.degree_anchors(ei, 3, 0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_host_formula_is_networkx():
    """The host expression the GPU tests compare with: NetworkX's degrees, and its scores bit for bit after the one multiplication
    engine.degree_centrality performs; a self-loop counts 2, a repeated edge once."""
    import networkx as nx
    ei, n = cli_graph()
    g = digraph(ei, n)
    deg = host_degrees(ei, n)
    assert deg.tolist() == [g.degree(v) for v in range(n)]
    dc = nx.degree_centrality(g)
    want = np.array([dc[v] for v in range(n)], dtype=np.float64)
    assert np.array_equal((deg.astype(np.float64) * (1.0 / (n - 1.0))).view(np.uint64), want.view(np.uint64))
    ranked = list({k: v for k, v in sorted(dc.items(), key=lambda item: item[1])}.keys())
    for k in (1, 12, n, n + 3, 0):
        assert host_anchors(ei, n, k) == ranked[-k:]
    assert host_degrees([[2], [2]], 4).tolist() == [0, 0, 2, 0]
    assert host_degrees([[0, 0, 0], [1, 1, 1]], 2).tolist() == [1, 1]
    assert nx.degree_centrality(digraph([[0], [0]], 1)) == {0: 1}


def test_without_a_gpu_the_host_branch_serves(monkeypatch):
    """sample_anchor_nodes keeps its NumPy branch for a machine without a GPU and never touches the engine there."""
    import torch
    from graphpope_amd import engine, utils as gp

    class D:
        pass
    ei, n = cli_graph()
    d = D()
    d.edge_index, d.num_nodes = torch.as_tensor(ei), n
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(engine, "degree_anchors", lambda *a, **k: pytest.fail("engine.degree_anchors called without a GPU"))
    for k in (12, 0, n + 3):
        assert gp.sample_anchor_nodes(d, k, "degree_centrality") == host_anchors(ei, n, k)


@pytest.mark.parametrize("n", SELECT_N)
def test_select_restatement_is_the_sorted_tail(n):
    """Digit-by-digit threshold search, compaction, fill with T and sort give np.sort(keys)[-K:] on every key set of the GPU test."""
    for k in select_ks(n, 4096):
        for name, keys in key_sets(n, k):
            assert keys.dtype == np.uint64 and keys.shape == (n,)
            assert np.array_equal(select_restated(keys, k), np.sort(keys)[-k:]), (name, k)


def test_key_sets_are_what_they_claim():
    n, k = 4097, 64
    sets = dict(key_sets(n, k))
    assert len(sets) == 11
    d = sets["distinct_full_range"]
    assert len(np.unique(d)) == n and abs(int((d >> np.uint64(63)).sum()) - n // 2) <= 1
    for byte in range(8):
        x = sets[f"byte_{byte}"] ^ sets[f"byte_{byte}"][0]
        assert (x & ~(np.uint64(0xFF) << np.uint64(8 * byte)) == 0).all() and len(np.unique(x)) > 100
    t = np.sort(sets["threshold_in_ties"])[-k]
    assert int((sets["threshold_in_ties"] > t).sum()) == k - 1 and int((sets["threshold_in_ties"] == t).sum()) == 500
