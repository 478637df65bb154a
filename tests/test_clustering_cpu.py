"""Clustering-coefficient anchors (utils.py:56-60 nx.clustering), the parts that need no GPU: the C ABI's argument checks and
scratch query, and the SciPy restatement the GPU tests compare the device counts with."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp


@pytest.fixture(autouse=True)
def _clean_error_string():
    """The library's error string is per thread and outlives a test: the rejected calls below would leave theirs to whichever
    test runs next in this process (test_abi reads it as empty).  A successful host-only call clears it."""
    yield
    from graphpope_amd import _lib
    buf = ctypes.create_string_buffer(64)
    _lib.check(_lib.load().pope_level_kernel_name(89250, 256, buf, 64))
    assert _lib.load().pope_last_error() == b""


def m_matrix(ei, n):
    """M = A + A^T as an int64 SciPy CSR, A the DiGraph's adjacency (repeated edges once) without self-loops."""
    src, dst = np.asarray(ei[0], dtype=np.int64), np.asarray(ei[1], dtype=np.int64)
    keep = src != dst
    a = sp.csr_matrix((np.ones(int(keep.sum()), dtype=np.int64), (src[keep], dst[keep])), shape=(n, n))
    a.sum_duplicates()
    a.data[:] = 1
    return (a + a.T).tocsr()


def restate_counts(m, rows=None, chunk=4096):
    """(T, dt, db) of the given rows (all by default): T = row sums of (M_rows @ M) * M_rows, row-chunked."""
    rows = np.arange(m.shape[0]) if rows is None else np.asarray(rows)
    t = np.zeros(len(rows), dtype=np.int64)
    for lo in range(0, len(rows), chunk):
        blk = m[rows[lo:lo + chunk]]
        t[lo:lo + chunk] = np.asarray((blk @ m).multiply(blk).sum(axis=1)).ravel()
    sub = m[rows]
    dt = np.asarray(sub.sum(axis=1)).ravel().astype(np.int64)
    db = np.diff(sub.indptr) - np.asarray((sub == 1).sum(axis=1)).ravel()
    return t, dt, db.astype(np.int64)


def networkx_formula(t, dt, db):
    """cluster.clustering's own expression, in Python ints: 0 if t == 0 else t / ((dt * (dt - 1) - 2 * db) * 2)."""
    return np.array([0.0 if int(a) == 0 else int(a) / ((int(b) * (int(b) - 1) - 2 * int(c)) * 2) for a, b, c in zip(t, dt, db)],
                    dtype=np.float64)


def digraph(ei, n):
    """The DiGraph utils._host_rankings scores (torch_geometric.utils.to_networkx(data))."""
    import networkx as nx
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(np.asarray(ei[0]).tolist(), np.asarray(ei[1]).tolist()))
    return g


def random_multigraph(n=300, e=2500, seed=5):
    """Directed, with repeated edges, reciprocal pairs and self-loops, in no particular order."""
    rs = np.random.RandomState(seed)
    src, dst = rs.randint(0, n, e), rs.randint(0, n, e)
    ei = np.stack([src, dst])
    ei = np.concatenate([ei, ei[:, :300], ei[::-1, 300:900], np.stack([np.arange(0, n, 7)] * 2)], axis=1)
    return ei[:, rs.permutation(ei.shape[1])].astype(np.int64), n


def test_restatement_is_networkx():
    """The SciPy restatement gives nx.clustering's float64 bits (directed multigraph with self-loops and reciprocal pairs)."""
    import networkx as nx
    ei, n = random_multigraph()
    t, dt, db = restate_counts(m_matrix(ei, n), chunk=64)
    want = nx.clustering(digraph(ei, n))
    assert np.array_equal(networkx_formula(t, dt, db), np.array([want[v] for v in range(n)]))
    assert (t % 2 == 0).all() and (db > 0).any()


def test_argument_validation_needs_no_gpu():
    """Null pointers, N <= 0, E < 0 and an E whose 2 E slots of M would wrap int32 are refused before any HIP call."""
    from graphpope_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(*ptrs, n=8, e=4, scratch_bytes=1 << 20):
        r, c, er, rt, ct, et, t, dt, db, s = ptrs
        return lib.pope_clustering_counts(r, c, er, rt, ct, et, n, e, t, dt, db, s, scratch_bytes, null)

    ok = [p] * 10
    for k in range(10):                                   # each pointer in turn
        args = list(ok)
        args[k] = null
        assert call(*args) == _lib.ERR_INVALID, k
        assert b"pope_clustering_counts" in lib.pope_last_error() and b"null pointer" in lib.pope_last_error()
    assert call(*ok, n=-1) == _lib.ERR_INVALID and b"pope_clustering_counts" in lib.pope_last_error()
    assert call(*ok, n=0) == _lib.ERR_INVALID
    assert call(*ok, n=1 << 31) == _lib.ERR_INVALID
    assert call(*ok, e=-1) == _lib.ERR_INVALID
    assert call(*ok, e=1 << 30) == _lib.ERR_INVALID                           # 2 E = 2^31: the offsets would wrap
    assert b"int32" in lib.pope_last_error() and b"pope_clustering_counts" in lib.pope_last_error()
    assert call(*ok, e=(1 << 31) - 1) == _lib.ERR_INVALID
    # with E == 0 the CSR column arrays are not needed, the outputs and scratch still are
    assert call(p, null, null, p, null, null, p, p, null, p, e=0) == _lib.ERR_INVALID
    # valid arguments: the scratch is sized next, by rocPRIM's queries for the current device.  A scratch smaller than that is
    # POPE_ERR_WORKSPACE; without a device the query itself fails and the call says so (POPE_ERR_HIP), it never guesses a size
    import torch
    want = _lib.ERR_WORKSPACE if torch.cuda.is_available() else _lib.ERR_HIP
    assert call(*ok, scratch_bytes=16) == want and b"pope_clustering_counts" in lib.pope_last_error()


def test_scratch_query_needs_no_gpu():
    """The query answers without a GPU: 0 for refused sizes, and 0 when no device is visible (rocPRIM sizes its temporaries for
    the current device: an answer without them would be too small); with a device, room for every part of the layout."""
    import torch
    from graphpope_amd import _lib
    lib = _lib.load()
    assert lib.pope_clustering_scratch_bytes(0, 10) == 0 and lib.pope_clustering_scratch_bytes(10, -1) == 0
    assert lib.pope_clustering_scratch_bytes(10, 1 << 30) == 0             # 2 E = 2^31 slots: refused
    flickr = lib.pope_clustering_scratch_bytes(89250, 899756)
    if not torch.cuda.is_available():
        assert flickr == 0 and lib.pope_clustering_scratch_bytes(1, 0) == 0
        return
    assert flickr >= 2 * 899756 * 9 + 2 * 899756 * 4                       # codes + scan, oriented rows unsorted + sorted
    assert lib.pope_clustering_scratch_bytes(1, 0) > 0
    assert lib.pope_clustering_scratch_bytes(89250, 2 * 899756) > flickr
    assert lib.pope_clustering_scratch_bytes(10, (1 << 30) - 1) > 0
