"""CPU-side checks of the gradient-clipping exports (include/graphpope_hip.h: sage_grad_norm_partials, sage_grad_sqnorm,
sage_adam_step_clip; main.py:285-290 gradient_clip_val=0.5): they load, the size query is host arithmetic, and bad arguments are
refused before any HIP call."""
import ctypes

ADAM_CHUNK, ADAM_MAX_TENSORS, CLIP_MAX_PARTS = 4096, 24, 256          # csrc/epilogue.hip


def _numel(values):
    return (ctypes.c_int64 * len(values))(*values)


def test_clip_symbols_load():
    from graphpope_amd import _lib
    lib = _lib.load()
    for name in ("sage_grad_norm_partials", "sage_grad_sqnorm", "sage_adam_step_clip"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_partial_count_is_chunks_clamped_to_the_bound():
    """clamp(sum of ceil(numel / 4096), 1, 256): one partial per chunk until the bound, which no model size moves."""
    from graphpope_amd import _lib
    lib = _lib.load()

    def parts(values):
        return lib.sage_grad_norm_partials(len(values), _numel(values))

    assert parts([1]) == 1 and parts([4096]) == 1 and parts([4097]) == 2
    assert parts([256 * 756, 256, 7 * 256, 5000, 27, 1, 4097]) == 48 + 1 + 1 + 2 + 1 + 1 + 2
    assert parts([0, 0]) == 1 and lib.sage_grad_norm_partials(0, None) == 1          # nothing to add up: one partial, zero
    many = [10] * (ADAM_MAX_TENSORS + 9)                                             # more tensors than one Adam launch describes
    assert parts(many) == ADAM_MAX_TENSORS + 9
    assert parts([10] * 300) == CLIP_MAX_PARTS                                       # more tensors than partials
    assert parts([ADAM_CHUNK * CLIP_MAX_PARTS]) == CLIP_MAX_PARTS
    assert parts([ADAM_CHUNK * CLIP_MAX_PARTS + 1]) == CLIP_MAX_PARTS                # above the bound: blocks stride over the chunks
    assert parts([1 << 40]) == CLIP_MAX_PARTS
    assert parts([5, -1]) == 0 and lib.sage_grad_norm_partials(-1, None) == 0 and lib.sage_grad_norm_partials(2, None) == 0
    assert lib.pope_last_error() == b""


def test_clip_argument_validation_needs_no_gpu():
    from graphpope_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below is refused before a launch
    one = (ctypes.c_void_p * 1)(4096)
    n1 = _numel([5 * ADAM_CHUNK])                      # 5 partials

    def step(max_norm, partials, n_partials, numel=n1, xent=(null, 0, null)):
        return lib.sage_adam_step_clip(1, one, one, one, one, numel, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, null, max_norm, partials, n_partials,
                                       null, xent[0], xent[1], xent[2], null)

    assert step(-0.5, fake, 5) == _lib.ERR_INVALID and b"max_norm" in lib.pope_last_error()
    assert step(float("nan"), fake, 5) == _lib.ERR_INVALID and b"max_norm" in lib.pope_last_error()
    assert step(0.5, null, 5) == _lib.ERR_INVALID and b"partials" in lib.pope_last_error()
    assert step(0.5, fake, 4) == _lib.ERR_INVALID and b"partials" in lib.pope_last_error()            # the query says 5
    assert step(0.5, fake, CLIP_MAX_PARTS + 1) == _lib.ERR_INVALID
    assert step(0.5, fake, 5, numel=_numel([-3])) == _lib.ERR_INVALID
    assert step(0.5, fake, 5, xent=(fake, 0, fake)) == _lib.ERR_INVALID                               # loss rows without a count
    assert step(0.5, fake, 5, xent=(fake, 8, null)) == _lib.ERR_INVALID
    assert lib.sage_adam_step_clip(2, null, null, null, null, _numel([1, 1]), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, null, 0.5, fake, 2, null, null, 0,
                                   null, null) == _lib.ERR_INVALID                                    # sage_adam_step's own checks still hold
    assert lib.sage_adam_step_clip(1, one, one, one, one, n1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, null, 0.5, fake, 5, null, null, 0, null,
                                   null) == _lib.ERR_INVALID                                          # step is 1-based
    assert lib.sage_grad_sqnorm(1, one, n1, null, 5, null) == _lib.ERR_INVALID and b"workspace" in lib.pope_last_error()
    assert lib.sage_grad_sqnorm(1, one, n1, fake, 4, null) == _lib.ERR_INVALID and b"workspace" in lib.pope_last_error()
    assert lib.sage_grad_sqnorm(1, null, n1, fake, 5, null) == _lib.ERR_INVALID
    assert lib.sage_grad_sqnorm(1, one, _numel([-1]), fake, 5, null) == _lib.ERR_INVALID
    assert lib.sage_grad_sqnorm(1, (ctypes.c_void_p * 1)(0), n1, fake, 5, null) == _lib.ERR_INVALID   # a tensor with elements and no address
