"""A caller-owned scratch buffer with guard bands, shared by tests/test_workspace_cpu.py and tests/test_workspace_gpu.py.  Not a test
module and not a conftest: the fixtures below are imported by the modules that use them.

Every kernel family takes a (scratch, scratch_bytes) pair that the caller sizes with a query (include/graphpope_hip.h).  The Python
layer hands over exactly the queried number of bytes from torch's caching allocator, and keeps many of those buffers alive across calls.
Two promises follow that a result-only test on fresh memory cannot see:

  contained           nothing is written in front of the buffer or behind the promised size -- GuardedScratch puts 4096 bytes of 0xA5 on
                      both sides (the guard size of the K-means, top-k, clustering and eigenvector tests) and compares them afterwards;
  self-initialising   nothing is read that the call did not write itself -- GuardedScratch.fill puts zeros, 0xFF, seeded random bytes or
                      the bytes another call left there into the buffer before the call, and the outputs must not move by a bit.

The third, `refused`: a scratch one byte short is turned down before anything is launched -- snapshot() / unchanged_since() show that
not a byte of it moved.  The short buffer is still the middle of the same allocation, so even a missing check cannot leave it."""
import ctypes

import numpy as np
import pytest
import torch

BAND = 4096
BAND_BYTE = 0xA5
FILLS = ("zeros", "ones", "noise", "keep")


class GuardedScratch:
    """One uint8 allocation of band + nbytes (rounded up to 256) + band bytes on `dev` (a torch device, CPU included).  The scratch is
    `view`: nbytes bytes that start `band` bytes in, 256-byte aligned like a buffer of the caching allocator, so no plan changes because
    of the wrapper (plans look at aligned16(scratch)).  The front band and everything from the end of the view on hold 0xA5: a write at
    view[-1] or at view[nbytes] breaks bands_intact()."""

    def __init__(self, dev, nbytes, band=BAND):
        self.nbytes, self.band = int(nbytes), int(band)
        assert self.nbytes >= 0 and self.band > 0 and self.band % 256 == 0
        self.rear = self.band + (self.nbytes + 255) // 256 * 256           # where the rear band starts
        # the caching allocator gives 256-byte alignment on the device (lo = band); a host allocation is shifted to it by hand
        slack = 0 if torch.device(dev).type == "cuda" else 256
        self.buf = torch.full((self.rear + self.band + slack,), BAND_BYTE, dtype=torch.uint8, device=dev)
        self.lo = (-self.buf.data_ptr()) % 256 + self.band
        assert self.lo + self.nbytes + self.band <= self.buf.numel()
        self.view = self.buf[self.lo:self.lo + self.nbytes]
        assert self.nbytes == 0 or self.view.data_ptr() % 256 == 0
        self._seed = 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.lo)

    def short(self, by=1):
        """(ptr, nbytes - by): the same buffer, promised `by` bytes shorter."""
        return self.ptr, self.nbytes - by

    def fill(self, kind):
        """zeros / ones (0xFF) / noise (seeded random bytes, new ones every time) / keep (whatever the previous call left)."""
        assert kind in FILLS, kind
        if kind == "zeros":
            self.view.zero_()
        elif kind == "ones":
            self.view.fill_(0xFF)
        elif kind == "noise":
            self._seed += 1
            noise = np.random.RandomState(1000 + self._seed).randint(0, 256, size=self.nbytes, dtype=np.uint8)
            self.view.copy_(torch.from_numpy(noise))
        return self

    def load(self, data):
        """The first bytes of the buffer take `data` (uint8, any device; what does not fit is dropped): another call's leftovers."""
        n = min(self.nbytes, int(data.numel()))
        self.view[:n].copy_(data[:n])
        return self

    def snapshot(self):
        return self.buf.cpu().numpy().copy()                                # synchronises with the stream the kernels ran on

    def bands_intact(self):
        now = self.buf.cpu().numpy()
        return bool((now[:self.lo] == BAND_BYTE).all() and (now[self.lo + self.nbytes:] == BAND_BYTE).all())

    def unchanged_since(self, snapshot):
        return bool(np.array_equal(self.buf.cpu().numpy(), snapshot))

    def contents(self):
        return self.view.clone()


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


@pytest.fixture(scope="module")
def lib():
    from graphpope_amd import _lib
    return _lib.load()
