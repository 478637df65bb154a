"""Operands at addresses that are 4-byte but not 16-byte aligned, with guard floats around them.  Not a test module and not a conftest.

include/graphpope_hip.h asks of a float operand the alignment of its element type only; every entry point tests its pointers for 16-byte
alignment and picks the scalar form of a kernel, template instance or plan when the test fails.  place() builds such an operand: the array
at element offset `off` of a buffer of its own that is otherwise full of SENTINEL, so that a vector access that rounded its address down
(or ran past the end) shows in the floats in front of or behind the view (guards_intact)."""
import numpy as np
import torch

SENTINEL = 12345.0
GUARD = 8                                                              # floats behind the view (in front of it: `off`)


def place(array, dev, off):
    """`array` (float32) on `dev` at element offset `off` of a SENTINEL-filled buffer of off + array.size + 8 floats: the view, which
    remembers its buffer.  The view's address is 4 * off bytes past a 16-byte boundary -- asserted, so a case cannot silently be aligned."""
    a = np.ascontiguousarray(array, dtype=np.float32)
    buf = torch.full((off + a.size + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == (4 * off) % 16 and view.is_contiguous()
    view.guard_buffer, view.guard_off = buf, off
    return view


def empty(shape, dev, off):
    """place() of zeros: an output or a buffer the test fills later."""
    return place(np.zeros(shape, dtype=np.float32), dev, off)


def guards_intact(view):
    """The floats in front of and behind a place()d view still hold the sentinel."""
    buf, off = view.guard_buffer, view.guard_off
    front, back = buf[:off], buf[off + view.numel():]
    assert back.numel() == GUARD
    return bool((front == SENTINEL).all()) and bool((back == SENTINEL).all())
