"""node2vec without a GPU: the four pope_n2v_* entry points refuse bad sizes and null pointers before any HIP call, the generator's
command line carries the eight hyper-parameters of /root/reference/generate_node2vec_embedding.py:23-25 as defaults, and the
Node2Vec constructor raises what PyG's raises (walk_length < context_size) and says that p/q-biased walks are not implemented."""
import ctypes

import pytest
import torch


def _bad(lib, name, code):
    from graphpope_amd import _lib
    assert code == _lib.ERR_INVALID, name
    msg = lib.pope_last_error()
    assert name.encode() in msg, (name, msg)
    return msg


def test_entry_points_validate_before_any_hip_call():
    from graphpope_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(64)                     # a non-null address that is never dereferenced: every call below fails validation first

    # pope_n2v_walks(rowptr, col, N, starts, B, B_neg, walk_length, seed, first_row, pos, neg, stream)
    assert b"null pointer" in _bad(lib, "pope_n2v_walks", lib.pope_n2v_walks(null, null, 10, null, 4, 0, 5, 1, 0, null, null, null))
    assert b"null pointer" in _bad(lib, "pope_n2v_walks", lib.pope_n2v_walks(one, one, 10, one, 4, 4, 5, 1, 0, one, null, null))
    assert b"walk_length" in _bad(lib, "pope_n2v_walks", lib.pope_n2v_walks(one, one, 10, one, 4, 0, 0, 1, 0, one, null, null))
    _bad(lib, "pope_n2v_walks", lib.pope_n2v_walks(one, one, 0, one, 4, 0, 5, 1, 0, one, null, null))
    _bad(lib, "pope_n2v_walks", lib.pope_n2v_walks(one, one, 10, one, 4, 5, 5, 1, 0, one, one, null))               # B_neg > B
    _bad(lib, "pope_n2v_walks", lib.pope_n2v_walks(one, one, 10, one, 4, 0, 5, 1, -1, one, null, null))             # first_row < 0

    # pope_n2v_windows(rows, R, len, context, windows, stream)
    assert b"null pointer" in _bad(lib, "pope_n2v_windows", lib.pope_n2v_windows(null, 3, 8, 4, null, null))
    assert b"context" in _bad(lib, "pope_n2v_windows", lib.pope_n2v_windows(one, 3, 8, 1, one, null))
    assert b"context" in _bad(lib, "pope_n2v_windows", lib.pope_n2v_windows(one, 3, 8, 9, one, null))

    # pope_n2v_loss_grad(emb, N, D, rows, R, len, context, negative, scale, loss_acc, grad, touched, stream)
    assert b"null pointer" in _bad(lib, "pope_n2v_loss_grad", lib.pope_n2v_loss_grad(null, 10, 128, null, 3, 8, 4, 0, 1.0, null, null, null, null))
    assert b"null pointer" in _bad(lib, "pope_n2v_loss_grad", lib.pope_n2v_loss_grad(one, 10, 128, one, 3, 8, 4, 0, 1.0, one, one, null, null))
    assert b"context" in _bad(lib, "pope_n2v_loss_grad", lib.pope_n2v_loss_grad(one, 10, 128, one, 3, 8, 1, 0, 1.0, one, one, one, null))
    assert b"context" in _bad(lib, "pope_n2v_loss_grad", lib.pope_n2v_loss_grad(one, 10, 128, one, 3, 8, 9, 0, 1.0, one, one, one, null))
    for d in (48, 0, 16, 288, 130):
        assert b"multiple of 32" in _bad(lib, "pope_n2v_loss_grad", lib.pope_n2v_loss_grad(one, 10, d, one, 3, 8, 4, 0, 1.0, one, one, one, null))
    assert b"LDS" in _bad(lib, "pope_n2v_loss_grad", lib.pope_n2v_loss_grad(one, 10, 256, one, 3, 100, 4, 0, 1.0, one, one, one, null))

    # pope_n2v_sparse_adam(emb, grad, touched, exp_avg, exp_avg_sq, N, D, lr, beta1, beta2, eps, step, stream)
    assert b"null pointer" in _bad(lib, "pope_n2v_sparse_adam", lib.pope_n2v_sparse_adam(null, null, null, null, null, 10, 128, 0.01, 0.9, 0.999, 1e-8, 1, null))
    assert b"step" in _bad(lib, "pope_n2v_sparse_adam", lib.pope_n2v_sparse_adam(one, one, one, one, one, 10, 128, 0.01, 0.9, 0.999, 1e-8, 0, null))
    assert b"multiple of 32" in _bad(lib, "pope_n2v_sparse_adam", lib.pope_n2v_sparse_adam(one, one, one, one, one, 10, 48, 0.01, 0.9, 0.999, 1e-8, 1, null))
    _bad(lib, "pope_n2v_sparse_adam", lib.pope_n2v_sparse_adam(one, one, one, one, one, 10, 128, 0.01, 1.0, 0.999, 1e-8, 1, null))

    # empty calls are fine and launch nothing
    assert lib.pope_n2v_walks(null, null, 10, null, 0, 0, 5, 1, 0, null, null, null) == _lib.OK
    assert lib.pope_n2v_windows(null, 0, 8, 4, null, null) == _lib.OK
    assert lib.pope_n2v_sparse_adam(null, null, null, null, null, 0, 128, 0.01, 0.9, 0.999, 1e-8, 1, null) == _lib.OK
    assert lib.pope_last_error() == b""


def test_generator_defaults_are_the_reference_scripts():
    from graphpope_amd.generate_node2vec_embedding import build_parser
    ns = vars(build_parser().parse_args([]))
    assert {k: ns[k] for k in ("embedding_dim", "walk_length", "context_size", "walks_per_node", "num_negative_samples", "p", "q",
                               "sparse")} == {"embedding_dim": 128, "walk_length": 20, "context_size": 10, "walks_per_node": 10,
                                              "num_negative_samples": 1, "p": 1, "q": 1, "sparse": True}
    assert ns["epochs"] == 0 and ns["seed"] == 42 and ns["batch_size"] == 128 and ns["lr"] == 0.01 and ns["out"] is None
    ns = build_parser().parse_args("--dataset flickr --epochs 3 --embedding_dim 64 --walk_length 8 --context_size 4 --walks_per_node 2 "
                                   "--num_negative_samples 2 --p 1 --q 1 --sparse false --batch_size 32 --lr 0.05 --seed 7 --out x.pt "
                                   "--data_dir d".split())
    assert (ns.dataset, ns.epochs, ns.embedding_dim, ns.walk_length, ns.context_size, ns.walks_per_node, ns.num_negative_samples) == \
        ("flickr", 3, 64, 8, 4, 2, 2)
    assert ns.sparse is False and ns.batch_size == 32 and ns.lr == 0.05 and ns.seed == 7 and ns.out == "x.pt" and ns.data_dir == "d"


def test_constructor_raises_before_it_needs_a_gpu():
    from graphpope_amd.node2vec import Node2Vec
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(AssertionError):
        Node2Vec(ei, 32, walk_length=3, context_size=4)
    for p, q in ((2, 1), (1, 0.5)):
        with pytest.raises(NotImplementedError, match="p = 1, q = 1"):
            Node2Vec(ei, 32, walk_length=5, context_size=3, p=p, q=q)
