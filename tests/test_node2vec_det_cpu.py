"""node2vec's deterministic pair without a GPU: pope_n2v_position_grads, pope_n2v_accumulate_det and its size query refuse bad sizes
and null pointers before any HIP call, the size query answers without a device, the NumPy restatement of the accumulate contract
(tests/node2vec_det_cases.py) is checked by hand, the inputs of the ordered-sum GPU test do tell orders apart, and the generator's
``main`` enters and leaves the mode under GRAPHPOPE_DETERMINISTIC=1.  Host logic only; every test leaves the switch off."""
import ctypes

import numpy as np
import pytest

import node2vec_det_cases as cases
from graphpope_amd import _lib

POSITION, ACCUMULATE = "pope_n2v_position_grads", "pope_n2v_accumulate_det"


@pytest.fixture
def lib():
    lib = _lib.load()
    assert lib.sage_get_deterministic() == 0, "an earlier test left the switch on"
    yield lib
    lib.sage_set_deterministic(0)
    null = ctypes.c_void_p(0)
    lib.pope_n2v_position_grads(null, 10, 128, null, 0, 8, 4, 0, 1.0, null, null, null, null)      # an empty call: leaves no message behind


def _refused(lib, name, good, code=None, **change):
    args = list(good)
    for k, v in change.items():
        args[int(k[1:])] = v
    assert getattr(lib, name)(*args) == (_lib.ERR_INVALID if code is None else code), (name, change)
    msg = lib.pope_last_error()
    assert name.encode() in msg, (name, change, msg)
    return msg


def test_position_grads_validates_before_any_hip_call(lib):
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)          # `one`: never dereferenced, every call below fails validation first
    # (emb, N, D, rows, R, len, context, negative, scale, ids, contrib, row_loss, stream)
    good = [one, 10, 128, one, 3, 8, 4, 0, 1.0, one, one, one, null]
    for at in (0, 3, 9, 10, 11):
        assert b"null pointer" in _refused(lib, POSITION, good, **{"a%d" % at: null})
    for d in (48, 288, 0, 16, 130):
        assert b"multiple of 32" in _refused(lib, POSITION, good, a2=d)
    for context in (1, 0, 9):                                    # < 2, > len
        assert b"context" in _refused(lib, POSITION, good, a6=context)
    _refused(lib, POSITION, good, a4=-1)                         # negative sizes
    _refused(lib, POSITION, good, a1=-1)
    _refused(lib, POSITION, good, a1=0)
    _refused(lib, POSITION, good, a1=2 ** 31)
    assert b"LDS" in _refused(lib, POSITION, good, a2=256, a5=100)
    assert lib.pope_n2v_position_grads(one, 2 ** 31 - 1, 256, null, 0, 8, 4, 1, 1.0, null, null, null, null) == _lib.OK
    assert lib.pope_n2v_position_grads(null, 10, 128, null, 0, 8, 4, 0, 1.0, null, null, null, null) == _lib.OK
    assert lib.pope_last_error() == b""


def test_accumulate_det_validates_before_any_hip_call(lib):
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    m, n = 20, 10
    room = lib.pope_n2v_accumulate_det_scratch_bytes(m, n)
    # (ids, M, contrib, D, N, grad, touched, row_loss, R, scale, loss_acc, scratch, scratch_bytes, stream)
    good = [one, m, one, 128, n, one, one, one, 3, 1.0, one, one, room, null]
    for at in (0, 2, 5, 6, 10, 11):                              # ids, contrib, grad, touched, loss_acc (with row_loss), scratch
        assert b"null pointer" in _refused(lib, ACCUMULATE, good, **{"a%d" % at: null})
    for d in (48, 288):
        assert b"multiple of 32" in _refused(lib, ACCUMULATE, good, a3=d)
    _refused(lib, ACCUMULATE, good, a1=-1)
    _refused(lib, ACCUMULATE, good, a8=-1)
    _refused(lib, ACCUMULATE, good, a4=0)
    _refused(lib, ACCUMULATE, good, a4=-1)
    _refused(lib, ACCUMULATE, good, a4=2 ** 31)
    _refused(lib, ACCUMULATE, good, a1=2 ** 31 - 1)
    assert b"scratch" in _refused(lib, ACCUMULATE, good, code=_lib.ERR_WORKSPACE, a12=room - 1)
    _refused(lib, ACCUMULATE, good, code=_lib.ERR_WORKSPACE, a12=0)
    # empty calls take null pointers and launch nothing
    assert lib.pope_n2v_accumulate_det(null, 0, null, 128, n, null, null, null, 0, 1.0, null, null, 0, null) == _lib.OK
    assert lib.pope_n2v_accumulate_det(null, 0, null, 128, n, null, null, null, 5, 1.0, null, null, 0, null) == _lib.OK   # no row_loss: no loss part
    assert lib.pope_n2v_accumulate_det(null, 0, null, 128, n, null, null, one, 0, 1.0, null, null, 0, null) == _lib.OK    # R = 0: none either
    assert lib.pope_last_error() == b""


def test_scratch_size_query_answers_without_a_device(lib):
    size = lib.pope_n2v_accumulate_det_scratch_bytes
    for m, n in ((1, 1), (20, 10), (3000, 70), (53760, 19717), (2 ** 31 - 2, 2 ** 31 - 1)):
        assert size(m, n) >= 4 * (n + 1) + 8 * m, (m, n)          # start [N + 1], list [M], sorted [M]: int32 each
    ms, ns = (0, 1, 2, 64, 65, 3000, 10 ** 6), (1, 2, 70, 10 ** 5, 2 ** 31 - 1)
    for n in ns:
        got = [size(m, n) for m in ms]
        assert got == sorted(got), n
    for m in ms:
        got = [size(m, n) for n in ns]
        assert got == sorted(got), m
    assert size(0, 70) == 0                                        # nothing to index
    for m, n in ((-1, 70), (10, 0), (10, -1), (10, 2 ** 31), (2 ** 31 - 1, 70)):
        assert size(m, n) == 0, (m, n)                             # refused sizes ask for nothing


def test_restatement_of_the_accumulate_contract_on_a_tiny_case():
    """3 nodes, 5 entries, one id -1, a non-zero prior: node 0 gets entries 0 and 3 in that order, node 2 entries 2 and 4, node 1 none."""
    ids = np.array([0, -1, 2, 0, 2], dtype=np.int32)
    big = np.float32(2.0 ** 80)
    half_ulp = np.float32(2.0 ** -24)                               # of 1.0f: 1.0f + 2^-24 rounds back to 1.0f
    contrib = np.array([[1.0, big], [50.0, 50.0], [0.25, half_ulp], [2.0, -big], [0.5, half_ulp]], dtype=np.float32)
    grad = np.array([[10.0, 1.0], [-7.0, -7.0], [0.125, 1.0]], dtype=np.float32)
    out, touched = cases.accumulate_reference(ids, contrib, grad)
    assert touched.tolist() == [1, 0, 1] and out.dtype == np.float32
    assert out[0].tolist() == [13.0, 1.0]                          # 10 + (1 + 2); 1 + (2^80 - 2^80)
    assert out[1].tolist() == [-7.0, -7.0]                         # no entry: untouched (the skipped entry's 50 went nowhere)
    assert out[2, 0] == np.float32(0.875)
    assert out[2, 1] == np.float32(1.0 + 2.0 ** -23)               # float64 sum, ONE rounding ...
    assert (grad[2, 1] + half_ulp) + half_ulp == np.float32(1.0)   # ... where float32 additions would have lost both terms
    assert grad[0, 0] == 10.0                                       # the input is not modified
    # the order is part of the contract: entry 3 before entry 0 changes nothing here, but around a swallowing term it does
    ids2 = np.zeros(3, dtype=np.int32)
    contrib2 = np.array([[1.0], [big], [-big]], dtype=np.float32)
    zero = np.zeros((1, 1), dtype=np.float32)
    assert cases.accumulate_reference(ids2, contrib2, zero)[0][0, 0] == 0.0                       # 1 is swallowed by 2^80
    assert cases.accumulate_reference(ids2, contrib2, zero, order=[2, 1, 0])[0][0, 0] == 1.0     # 1 arrives after the pair has gone


@pytest.mark.parametrize("d", [32, 96, 128, 256])
def test_inputs_of_the_ordered_sum_test_tell_orders_apart(d):
    """Descending entry order gives another float32 result than ascending for at least 90 % of the lists (one list: one node, one
    column) of the very case the GPU test runs; the same lists without the crafted pairs show no difference at all."""
    ids, contrib, grad = cases.ordered_sum_case(d)
    up, touched = cases.accumulate_reference(ids, contrib, grad)
    down, _ = cases.accumulate_reference(ids, contrib, grad, order=range(len(ids) - 1, -1, -1))
    lists = touched.astype(bool)
    assert lists.sum() >= 40 and np.isfinite(up).all() and np.isfinite(down).all()
    differ = (up[lists].view(np.int32) != down[lists].view(np.int32)).mean()
    print(f"D = {d}: {differ:.4f} of {lists.sum() * d} lists differ between ascending and descending order")
    assert differ >= 0.90
    assert np.array_equal(up[~lists].view(np.int32), grad[~lists].view(np.int32))
    plain = np.random.default_rng(1).standard_normal(contrib.shape).astype(np.float32)
    a, _ = cases.accumulate_reference(ids, plain, grad)
    b, _ = cases.accumulate_reference(ids, plain, grad, order=range(len(ids) - 1, -1, -1))
    assert (a.view(np.int32) != b.view(np.int32)).mean() < 0.01


@pytest.mark.parametrize("env, inside", [("1", True), ("0", False), (None, False)])
def test_generator_main_enters_and_leaves_the_mode(lib, monkeypatch, env, inside):
    """GRAPHPOPE_DETERMINISTIC=1: load_dataset and Node2Vec run inside the mode; it is off again afterwards, also when the run ends in
    an exception (the stub model's way out: nothing behind its construction runs without a GPU)."""
    import torch
    from graphpope_amd import generate_node2vec_embedding as gen, main as gp_main, sage
    seen = []

    class Stop(Exception):
        pass

    class Edges:
        def to(self, *a, **k):
            return self

    class Data:
        edge_index, num_nodes = Edges(), 4

    def load_dataset(name, data_dir):
        seen.append(("load_dataset", sage.is_deterministic()))
        return Data(), 3

    def node2vec(*a, **k):
        seen.append(("Node2Vec", sage.is_deterministic()))
        raise Stop

    monkeypatch.setattr(gp_main, "load_dataset", load_dataset)
    monkeypatch.setattr(gen, "Node2Vec", node2vec)
    monkeypatch.setattr(torch.cuda, "set_device", lambda dev: None)
    if env is None:
        monkeypatch.delenv("GRAPHPOPE_DETERMINISTIC", raising=False)
    else:
        monkeypatch.setenv("GRAPHPOPE_DETERMINISTIC", env)
    with pytest.raises(Stop):
        gen.main(["--dataset", "pubmed", "--epochs", "1", "--data_dir", "nowhere"])
    assert seen == [("load_dataset", inside), ("Node2Vec", inside)]
    assert sage.is_deterministic() is False
