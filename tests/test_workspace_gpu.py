"""What every entry point promises about the scratch buffer its caller owns, row by row of tests/workspace_cases.py, each on a
GuardedScratch (tests/workspace.py) of EXACTLY the size its query answers:

  contained           the call gives its reference result (the comparison of the entry point's own test: bit equality wherever the inputs
                      are the exact family or the kernel is deterministic) and both 4096-byte bands around the buffer are intact;
  self_initialising   the same call on a buffer full of zeros, of 0xFF, of random bytes and of what a different, larger call of the same
                      entry point left in its scratch (those bytes, copied to the same offsets) gives the same bits in every output.  The two paths that add with float atomics -- the
                      atomic scatter of the SAGE backward pass is the one that has a scratch -- run on the exact family, so the order of
                      the additions cannot matter;
  refused             one byte less (and, where the call needs scratch, a null pointer): the code include/graphpope_hip.h documents,
                      pope_last_error() naming both sizes, every output still at its sentinel and not a byte of the buffer changed --
                      nothing was launched.  The sage_conv_forward* calls are the documented exception: with less scratch (one byte
                      less, none) forward_plan takes other kernels, the result and the bands stay.

The sampler is the one family whose kernels WAIT on words of the scratch, so a fill could stall it instead of changing its result.
Read in csrc/sampler.hip before these tests first ran, which launch initialises each word a wait reads:
  * chain_prefix spins on status[j] until (w >> 32) != 0, for tickets j below its own, in k_sample_count_scan and
    k_sample_rank_relabel.  The status words and the two tickets of hop 0 are zeroed by k_sample_begin, the first launch of every
    sage_sample_hop call and of a batch; those of hop h + 1 lie in the other region and are zeroed by hop h's k_sample_count_scan
    (clear_region on next_words), one launch ahead of the first kernel that draws a ticket there.  A block publishes its own word before
    it reads the lower ones, and a lower ticket was drawn by a block that is running or done: a zero word is always on its way.
  * k_sample_rank_relabel spins on rank[p0] until it is >= 0, for the slot p0 < nnz at which the node was first picked.  Every slot
    p < nnz gets rank[p] = -1 from k_sample_pick (k_sample_all for fan-out -1) of the same hop, the launch before, and its final value
    from the block that owns it, which drew a lower or the same ticket.
  So neither zeros nor 0xFF (a published status word, a rank of -1 ...) can be read by a wait before the call has overwritten it.

Every GPU step of a run of this file gets a time limit from the command that starts it."""
import pytest
import torch

import workspace_cases as wc
from workspace import FILLS, GuardedScratch, dev, lib  # noqa: F401  (the fixtures live in the helper module)

pytestmark = pytest.mark.gpu

_built = {}                                         # row id -> Call: one row's operands serve its three tests
_leftovers = {}                                     # row id -> what the row's call left in its scratch (uint8, host)


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    """A fault is sticky: every later call in the process would fail the same way.  The run ends at the test that met it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the GPU reported an error, nothing more is started: %s" % e, returncode=3)


def _call(row, dev, lib):
    """The row's Call, built under the row's knobs (the caller holds row.context); only the latest row is kept."""
    if row.id not in _built:
        _built.clear()
        _built[row.id] = row.make(dev, lib)
        assert _built[row.id].entry == row.entry
    return _built[row.id]


def _same_bits(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


def _run_ok(call, guard):
    """One accepted call on the guarded buffer: code 0, the outputs (also checked against the reference), every band intact."""
    from graphpope_amd import _lib
    call.reset()
    rc = call.run(guard.ptr, guard.nbytes)
    assert rc == 0, (rc, _lib.load().pope_last_error())
    out = call.outputs()
    call.check(out)
    assert guard.bands_intact(), "the call wrote in front of its scratch or behind the %d bytes its query asked for" % guard.nbytes
    for g in call.guards:
        assert g.bands_intact(), "the call wrote outside an output of the size the header states"
    return out


def _leftover_of(donor, dev, lib):
    """What the donor row's call leaves in a scratch of its own size (run once, under the donor's knobs)."""
    if donor.id not in _leftovers:
        with donor.context(lib):
            other = donor.make(dev, lib)
            guard = GuardedScratch(dev, other.need)
            guard.fill("noise")
            other.reset()
            assert other.run(guard.ptr, guard.nbytes) == 0
            torch.cuda.synchronize()
            _leftovers[donor.id] = guard.contents().cpu()
    return _leftovers[donor.id]


def _ids(rows):
    return [r.id for r in rows]


_CONTAINED = [r for r in wc.ROWS if "contained" in r.props]
_SELF_INIT = [r for r in wc.ROWS if "self_initialising" in r.props]
_REFUSED = [r for r in wc.ROWS if "refused" in r.props]


@pytest.mark.parametrize("row", _CONTAINED, ids=_ids(_CONTAINED))
def test_the_queried_size_is_enough_and_nothing_is_written_outside_it(row, dev, lib):
    with row.context(lib):
        call = _call(row, dev, lib)
        assert call.need >= 0 and (call.need > 0 or call.runs_with_less), "a call that needs scratch must be told how much"
        guard = GuardedScratch(dev, call.need)
        assert call.need == 0 or guard.view.data_ptr() % 256 == 0
        _run_ok(call, guard)


@pytest.mark.parametrize("row", _SELF_INIT, ids=_ids(_SELF_INIT))
def test_the_result_does_not_depend_on_what_the_scratch_held(row, dev, lib):
    donor = wc.donor_of(row)
    left = _leftover_of(donor, dev, lib) if donor is not None else None
    with row.context(lib):
        call = _call(row, dev, lib)
        if call.need == 0:
            return                                                   # no scratch, nothing to fill
        guard = GuardedScratch(dev, call.need)
        first = _run_ok(call, guard)
        for kind in FILLS:
            if kind == "keep" and left is not None:                  # the bytes a different, larger call of this entry point left behind
                guard.load(left.to(dev))
            guard.fill(kind)
            again = _run_ok(call, guard)
            assert _same_bits(first, again), (kind, [k for k in first if first[k].tobytes() != again[k].tobytes()])


@pytest.mark.parametrize("row", _REFUSED, ids=_ids(_REFUSED))
def test_a_scratch_that_is_too_small_is_refused_before_anything_is_launched(row, dev, lib):
    with row.context(lib):
        call = _call(row, dev, lib)
        if call.need == 0:
            return                                                   # the call takes no scratch: nothing to be short of
        guard = GuardedScratch(dev, call.need)
        guard.fill("noise")
        if call.runs_with_less:                                      # sage_conv_forward*: other kernels, the same result
            for ptr, nbytes in (guard.short(1), (guard.ptr, 0), (None, 0)):
                before = guard.snapshot()
                call.reset()
                assert call.run(ptr, nbytes) == 0, (nbytes, lib.pope_last_error())
                call.check(call.outputs())
                assert guard.bands_intact()
                if nbytes == 0:
                    assert guard.unchanged_since(before), "a call that was given no scratch wrote into it"
            return
        for ptr, nbytes, code in (guard.short(1) + (call.refusal,), (None, call.need, call.null_refusal), (None, 0, call.null_refusal)):
            before = guard.snapshot()
            call.reset()
            rc = call.run(ptr, nbytes)
            assert rc == code, (rc, code, nbytes, lib.pope_last_error())
            message = lib.pope_last_error().decode()
            if ptr is not None:                                      # the message names what it got and what it needs
                assert str(nbytes) in message and str(call.need) in message, message
            else:
                assert message, "a refusal without a message"
            assert call.untouched(), "a refused call wrote an output"
            assert guard.unchanged_since(before), "a refused call wrote into the scratch: something was launched"
            assert all(g.bands_intact() for g in call.guards)
        _run_ok(call, guard)                                         # and the next call with the promised size is served


@pytest.mark.parametrize("nbytes", [1, 292, 4096, 70001])
def test_guarded_scratch_on_the_device_sees_a_byte_on_either_side(nbytes, dev):
    """The helper itself on device memory (tests/test_workspace_cpu.py has it on host memory): the view starts one band into ONE
    allocation, 256-byte aligned as a buffer of the caching allocator is, and a byte written at view[-1] or at view[nbytes] -- inside the
    allocation the test owns -- turns bands_intact() false; a write inside the view does not."""
    g = GuardedScratch(dev, nbytes)
    assert g.lo == g.band and g.view.data_ptr() == g.buf.data_ptr() + g.band and g.view.data_ptr() % 256 == 0
    assert g.buf.numel() == 2 * g.band + (nbytes + 255) // 256 * 256
    for kind in FILLS:
        g.fill(kind)
        assert g.bands_intact()
    before = g.snapshot()
    g.view[nbytes - 1] = 1 + int(g.view[nbytes - 1]) % 200
    assert g.bands_intact() and not g.unchanged_since(before)
    for at in (g.lo - 1, g.lo + nbytes, 0, g.buf.numel() - 1):
        h = GuardedScratch(dev, nbytes)
        h.buf[at] = 0
        assert not h.bands_intact(), at


def test_clustering_scratch_query_on_the_device(dev, lib):
    """pope_clustering_scratch_bytes sizes rocPRIM's temporaries for the current device, so its part of tests/test_workspace_cpu.py runs
    here: 0 for sizes pope_clustering_counts rejects, positive otherwise, and non-decreasing while N or E doubles up to the documented
    limit E <= 2^30 - 1 (2 E must fit int32 offsets)."""
    q = lib.pope_clustering_scratch_bytes
    assert q(0, 4) == 0 and q(-1, 4) == 0 and q(5, -1) == 0 and q(5, 2 ** 30) == 0 and q(2 ** 31, 4) == 0
    base = (199, 396)
    assert q(*base) > 0
    for i, limit in ((0, 2 ** 31 - 2), (1, 2 ** 30 - 1)):
        args, prev = list(base), q(*base)
        while args[i] * 2 <= limit:
            args[i] *= 2
            now = q(*args)
            assert now >= prev > 0, (args, prev, now)
            prev = now
