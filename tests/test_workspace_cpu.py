"""The host side of the scratch promises (include/graphpope_hip.h): the GuardedScratch helper of tests/workspace.py tested on CPU
tensors, and every scratch size query -- what it answers for arguments its call rejects, that it never drops while an argument grows up
to the call's limit, and the lower bounds the header states.  No GPU: the queries are host arithmetic (pope_clustering_scratch_bytes,
which asks rocPRIM about the current device, has its part in tests/test_workspace_gpu.py)."""
import ctypes

import pytest
import torch

import workspace_cases as wc
from workspace import BAND, FILLS, GuardedScratch


@pytest.fixture(scope="module")
def lib():
    from graphpope_amd import _lib
    return _lib.load()


# ---- the helper ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [0, 1, 255, 256, 257, 5000])
def test_guarded_scratch_sees_a_byte_on_either_side(nbytes):
    cpu = torch.device("cpu")
    g = GuardedScratch(cpu, nbytes)
    assert g.nbytes == nbytes and g.view.numel() == nbytes and g.ptr.value % 256 == 0 and g.lo >= BAND
    assert g.buf.numel() >= BAND + (nbytes + 255) // 256 * 256 + BAND and g.bands_intact()
    assert nbytes == 0 or g.view.data_ptr() == g.ptr.value
    assert g.short(1)[1] == nbytes - 1 and g.short(1)[0].value == g.ptr.value
    snap = g.snapshot()
    for kind in FILLS:                                               # fills stay inside the view
        g.fill(kind)
        assert g.bands_intact()
    if nbytes:
        g.fill("zeros")
        assert not g.view.any()
        g.fill("ones")
        assert bool((g.view == 0xFF).all())
        a = g.fill("noise").contents()
        b = g.fill("noise").contents()
        assert nbytes < 8 or (not torch.equal(a, b) and len(a.unique()) > 1)
        assert torch.equal(g.fill("keep").contents(), b)            # keep: whatever the previous case left
        g.load(torch.arange(7, dtype=torch.uint8))
        assert g.view[:7].tolist() == list(range(7))[:nbytes] and g.bands_intact()
        assert not g.unchanged_since(snap)
    # one byte at -1 and one at nbytes, through the raw address as a kernel would write them
    for offset in (-1, nbytes):
        h = GuardedScratch(cpu, nbytes)
        before = h.snapshot()
        assert h.bands_intact() and h.unchanged_since(before)
        ctypes.c_uint8.from_address(h.ptr.value + offset).value = 0
        assert not h.bands_intact() and not h.unchanged_since(before), offset
    # ... and the far ends of both bands
    for offset in (-BAND, (nbytes + 255) // 256 * 256 + BAND - 1):
        h = GuardedScratch(cpu, nbytes)
        ctypes.c_uint8.from_address(h.ptr.value + offset).value = 0
        assert not h.bands_intact(), offset


def test_table_has_a_row_for_every_entry_point_that_takes_scratch():
    """The entry points the table must hold, and per entry point two rows of different weight wherever `keep` needs a different,
    larger call to inherit from."""
    entries = {r.entry for r in wc.ROWS}
    assert entries == {
        "sage_conv_forward", "sage_conv_forward_indexed", "sage_conv_forward_stats", "sage_conv_forward_indexed_stats",
        "sage_conv_backward", "sage_conv_backward_indexed", "sage_scatter_mean_det",
        "sage_bn_relu_dropout_forward", "sage_bn_relu_dropout_forward_stats", "sage_bn_relu_dropout_backward", "sage_bn_relu_dropout_backward_bias",
        "sage_sample_hop", "sage_sample_batch", "sage_sample_batch_device", "sage_sample_epoch_batch_device",
        "pope_csr_build", "pope_csr_build_canonical", "pope_geodesic_bfs", "pope_geodesic_bfs_begin+finish", "pope_geodesic_run",
        "pope_geodesic_column_stats", "pope_pairwise_features", "pope_pairwise_features_by_id", "pope_pairwise_minmax",
        "pope_betweenness_batch", "pope_n2v_accumulate_det", "pope_logreg_loss_grad"}
    for r in wc.ROWS:
        donor = wc.donor_of(r)
        assert set(r.props) <= set(wc.PROPS) and "contained" in r.props
        if "self_initialising" in r.props and len([o for o in wc.ROWS if o.entry == r.entry]) > 1:
            assert donor is not None and donor is not r and donor.entry == r.entry


def test_every_knob_a_row_sets_is_restored(lib):
    from graphpope_amd import _lib
    calls = []
    real = lib.pope_debug_set

    class Recorder:
        def __getattr__(self, name):
            return getattr(lib, name)

        def pope_debug_set(self, knob, value):
            calls.append((knob, value))
            return real(knob, value)

    for r in wc.ROWS:
        del calls[:]
        with pytest.raises(ZeroDivisionError):
            with r.context(Recorder()):
                assert lib.sage_get_deterministic() == int(r.det)
                1 / 0                                                  # the `finally` restores after a failure, too
        assert lib.sage_get_deterministic() == 0
        assert calls == [(getattr(_lib, k), v) for k, v, _ in r.knobs] + [(getattr(_lib, k), d) for k, _, d in r.knobs], r.id


# ---- the size queries ------------------------------------------------------------------------------------------------------------------
BIG = 2 ** 31 - 2            # sizes are "< 2^31" (most calls: < 2^31 - 1)
# query: (base arguments = the table's smallest shape, per argument the limit up to which it doubles (a callable sees the arguments),
#         arguments the call rejects and the query answers with 0)
QUERIES = {
    "pope_csr_scratch_bytes": ((50, 255), (BIG, BIG), [(-1, 4), (4, -1)]),
    "pope_csr_aux_elems": ((255,), (BIG,), [(-1,)]),
    "pope_betweenness_scratch_bytes": ((199, 1), (lambda a: min(BIG, 2 ** 40 // a[1]), lambda a: a[0]),
                                       [(0, 1), (-1, 1), (2 ** 31, 1), (5, 0), (5, 6), (2 ** 21, 2 ** 21)]),
    "pope_plane_bytes": ((201, 1), (BIG, BIG), [(-1, 1), (5, 0), (5, -1)]),
    "pope_bfs_scratch_bytes": ((201, 400, 1), (BIG, BIG, BIG), [(-1, 4, 1), (5, -1, 1), (5, 4, 0)]),
    "pope_geodesic_run_workspace_bytes": ((201, 400, 6, 8), (BIG, BIG, BIG, 31), [(5, -1, 1, 8), (5, 4, 0, 8), (5, 4, 1, 0), (5, 4, 1, 32)]),
    "pope_column_stats_scratch_bytes": ((1,), (BIG,), [(0,), (-1,)]),
    "pope_pairwise_scratch_bytes": ((33, 5, 4), (BIG, BIG, BIG), [(0, 5, 4), (-1, 5, 4), (33, 0, 4)]),
    "pope_pairwise_by_id_scratch_bytes": ((33, 5, 4), (BIG, BIG, BIG), [(0, 5, 4), (-1, 5, 4), (33, 0, 4), (33, 5, 0)]),
    "sage_conv_scratch_bytes": ((556, 256, 1000, 64, 64), (BIG, lambda a: a[0], BIG, BIG, BIG), [(0, 0, 0, 4, 4), (5, 5, 1, 0, 4), (5, 5, 1, 4, 0)]),
    "sage_conv_backward_indexed_scratch_bytes": ((2330, 1030, 4000, 40, 24), (BIG, lambda a: a[0], BIG, BIG, BIG),
                                                 [(0, 0, 0, 4, 4), (5, 5, 1, 0, 4), (5, 5, 1, 4, 0)]),
    "sage_conv_forward_scratch_bytes": ((515, 37, 30), (BIG, BIG, BIG), [(0, 4, 4), (-1, 4, 4), (5, 0, 4), (5, 4, 0)]),
    "sage_conv_forward_indexed_scratch_bytes": ((515, 37, 30), (BIG, BIG, BIG), [(0, 4, 4), (-1, 4, 4), (5, 0, 4), (5, 4, 0)]),
    "sage_scatter_mean_det_scratch_bytes": ((300, 130, 600), (BIG, lambda a: a[0], BIG), [(-1, 0, 0), (5, 6, 1), (5, 5, -1), (2 ** 31, 5, 1)]),
    "sage_sample_scratch_bytes": ((5, 1, 4), (BIG, BIG, BIG), [(0, 1, 4), (5, 0, 4), (5, 1, -1)]),
    "sage_bn_scratch_bytes": ((5,), (BIG,), [(0,), (-1,)]),
    "pope_n2v_accumulate_det_scratch_bytes": ((1, 70), (BIG, BIG), [(0, 70), (-1, 70), (5, 0), (5, 2 ** 31), (2 ** 31 - 1, 70)]),
    "pope_logreg_scratch_bytes": ((1, 33, 2), (2 ** 38 - 1, BIG, 64), [(0, 33, 2), (-1, 33, 2), (5, 0, 2), (5, 33, 1), (5, 33, 65), (2 ** 38, 33, 2)]),
    # the families whose own tests hold both promises already: the queries belong here all the same
    "pope_eigenvector_scratch_bytes": ((5,), (BIG,), [(0,), (-1,), (2 ** 31 - 1,)]),
    "pope_topk_scratch_bytes": ((5000, 1), (BIG, lambda a: min(a[0], 4096)), [(0, 1), (5, 0), (5, 6), (2 ** 31, 1), (10000, 4097)]),
    "pope_topk_f64_scratch_bytes": ((5000, 1), (BIG, lambda a: min(a[0], 4096)), [(0, 1), (5, 0), (5, 6), (2 ** 31, 1), (10000, 4097)]),
    "pope_kmeans_scratch_bytes": ((5, 4, 1), (BIG, BIG, BIG), [(0, 4, 1), (-1, 4, 1), (5, 0, 1), (5, 4, 0)]),
}


def test_every_scratch_query_of_the_header_is_in_the_table(lib):
    from graphpope_amd import _lib
    named = {n for n in _lib.SIGNATURES if n.endswith(("_scratch_bytes", "_workspace_bytes")) or n in ("pope_csr_aux_elems", "pope_plane_bytes")}
    assert named == set(QUERIES) | {"pope_clustering_scratch_bytes"}            # (that one: tests/test_workspace_gpu.py)


@pytest.mark.parametrize("name", list(QUERIES))
def test_a_size_query_answers_zero_for_arguments_its_call_rejects(name, lib):
    """Zero for every rejected size the header promises it for (betweenness, top-k, eigenvector, the inverted index of
    pope_n2v_accumulate_det, logreg) and for the sizes every other query answers with zero today: the non-positive ones, and for the
    deterministic sum n_dst > n_src and sizes of 2^31 as well.  (For sizes beyond 31 bits the CSR, BFS, run, SAGE and sampler queries
    go on computing a layout; the header promises nothing there, their calls refuse such sizes themselves.)  Positive at the base."""
    base, _, rejected = QUERIES[name]
    q = getattr(lib, name)
    assert q(*base) > 0 or name == "sage_conv_forward_scratch_bytes"             # (0 for small layers: scratch may be NULL then)
    for args in rejected:
        assert q(*args) == 0, args


@pytest.mark.parametrize("name", list(QUERIES))
def test_a_size_query_never_drops_while_an_argument_doubles(name, lib):
    """Each argument doubled from the base up to the call's documented limit, the others fixed: the answer is non-decreasing and, past
    the base, never 0 -- a 32-bit product that wrapped on the way would show as a drop.  (Run on this build for every query: none
    drops; the test pins that.  One query is not monotone by design, outside this sweep: pope_geodesic_run_workspace_bytes holds a region
    for the level-1 hit lists only up to 256 anchors and 262 144 nodes, so at a plane capacity of 1 or 2, where the planes are small
    beside it, the answer for 384 anchors is below the one for 192.)"""
    base, limits, _ = QUERIES[name]
    q = getattr(lib, name)
    for i, limit in enumerate(limits):
        args, prev, steps = list(base), q(*base), 0
        while args[i] * 2 <= (limit(args) if callable(limit) else limit):
            args[i] *= 2
            now = q(*args)
            assert now >= prev and (now > 0 or prev == 0), (name, tuple(args), prev, now)
            prev, steps = now, steps + 1
        assert steps >= (15 if limit == BIG else 1), (name, i, steps)
        assert prev < 2 ** 62


def test_sample_batch_checks_its_scratch_by_capacity_before_the_first_hop(lib):
    """sage_sample_batch sizes its scratch by the capacity of the last hop, t_cap[last] = n_seeds (1 + f0) ..., not by the counts the
    hops return: one byte less is POPE_ERR_WORKSPACE with both sizes in the message, before any HIP call (none could succeed here).
    4 seeds, fan-outs [25, 10]: t_cap = [4, 104], capacity of the last hop 1 040 edges."""
    from graphpope_amd import _lib
    fake = ctypes.c_void_p(4096)                                    # never dereferenced
    arr, fan = (ctypes.c_void_p * 2)(4096, 4096), (ctypes.c_int32 * 2)(25, 10)
    counts = (ctypes.c_int64 * 2)()
    need = lib.sage_sample_scratch_bytes(6600, 104, 1040)
    assert need > lib.sage_sample_scratch_bytes(6600, 4, 100) > 0
    for given in (need - 1, lib.sage_sample_scratch_bytes(6600, 4, 100), 0):
        assert lib.sage_sample_batch(fake, fake, 6600, fake, 4, fan, 2, 7, arr, arr, arr, counts, counts, fake, given, None) == _lib.ERR_WORKSPACE
        message = lib.pope_last_error().decode()
        assert str(given) in message and str(need) in message, message
    assert lib.sage_sample_batch(fake, fake, 6600, fake, 4, fan, 2, 7, arr, arr, arr, counts, counts, None, need, None) == _lib.ERR_INVALID


def test_lower_bounds_the_header_documents(lib):
    """pope_betweenness_scratch_bytes: 36 bytes per (source, node) "and change"; pope_n2v_accumulate_det_scratch_bytes: 4 (N + 1) + 8 M,
    the inverted index; pope_column_moments has no query: it refuses less than its 256 slabs of two float64 rows (256 * 2 * D * 8)."""
    from graphpope_amd import _lib
    for n, batch in ((199, 1), (199, 7), (199, 199), (89250, 8192), (2 ** 19, 2 ** 19)):
        need = lib.pope_betweenness_scratch_bytes(n, batch)
        assert need >= 36 * n * batch, (n, batch, need)
    for m, n in ((1, 70), (200, 70), (3000, 70), (53760, 89250), (2 ** 31 - 2, 2 ** 31 - 1)):
        assert lib.pope_n2v_accumulate_det_scratch_bytes(m, n) == 4 * (n + 1) + 8 * m, (m, n)
    fake = ctypes.c_void_p(4096)                                    # never dereferenced: the call below is refused before any HIP call
    for d in (1, 32, 128):
        least = 256 * 2 * d * 8
        assert lib.pope_column_moments(fake, 100, d, fake, fake, fake, least - 1, None) == _lib.ERR_INVALID
        assert b"scratch" in lib.pope_last_error()
