"""Second-order (p, q) node2vec walks without a GPU: pope_n2v_walks_biased refuses bad arguments before any HIP call,
SecondOrderNode2Vec refuses bad p and q before it needs a GPU, the generator's parser keeps the reference's defaults -- and the NumPy
restatement of the kernel's scheme (tests/node2vec_biased_cases.py), on its own, draws the node2vec distribution and reaches both of
its branches on the inputs of tests/test_node2vec_biased_gpu.py, so that bit-equality there carries these properties to the kernel."""
import ctypes

import numpy as np
import pytest
import torch

import node2vec_biased_cases as cases


def _bad(lib, code):
    from graphpope_amd import _lib
    assert code == _lib.ERR_INVALID
    msg = lib.pope_last_error()
    assert b"pope_n2v_walks_biased" in msg, msg
    return msg


def test_entry_point_validates_before_any_hip_call():
    from graphpope_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(64)                     # a non-null address that is never dereferenced: every call below fails validation first
    f = lib.pope_n2v_walks_biased                 # (rowptr, col, N, starts, B, walk_length, seed, first_row, p, q, pos, stream)
    _bad(lib, f(one, one, 0, one, 4, 5, 1, 0, 1.0, 1.0, one, null))                                  # N < 1
    _bad(lib, f(one, one, 1 << 31, one, 4, 5, 1, 0, 1.0, 1.0, one, null))                            # N >= 2^31
    assert b"walk_length" in _bad(lib, f(one, one, 10, one, 4, 0, 1, 0, 1.0, 1.0, one, null))
    _bad(lib, f(one, one, 10, one, -1, 5, 1, 0, 1.0, 1.0, one, null))                                # B < 0
    _bad(lib, f(one, one, 10, one, 4, 5, 1, -1, 1.0, 1.0, one, null))                                # first_row < 0
    for p, q in ((0.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (1.0, -1.0), (float("inf"), 1.0), (1.0, float("inf")), (float("nan"), 1.0),
                 (1.0, float("nan"))):
        assert b"finite" in _bad(lib, f(one, one, 10, one, 4, 5, 1, 0, p, q, one, null)), (p, q)
    for args in ((null, one, one, one), (one, null, one, one), (one, one, null, one), (one, one, one, null)):
        rowptr, col, starts, pos = args
        assert b"null pointer" in _bad(lib, f(rowptr, col, 10, starts, 4, 5, 1, 0, 2.0, 0.5, pos, null))
    # an empty call is fine with null pointers and launches nothing
    assert f(null, null, 10, null, 0, 5, 1, 0, 2.0, 0.5, null, null) == _lib.OK
    assert lib.pope_last_error() == b""


def test_second_order_constructor_raises_before_it_needs_a_gpu():
    from graphpope_amd.node2vec import Node2Vec, SecondOrderNode2Vec
    assert issubclass(SecondOrderNode2Vec, Node2Vec)
    ei = torch.tensor([[0, 1], [1, 0]])
    for p, q in ((0, 1), (1, -1), (float("inf"), 1), (1, float("inf")), (float("nan"), 1), (1, float("nan"))):
        with pytest.raises(ValueError):
            SecondOrderNode2Vec(ei, 32, walk_length=5, context_size=3, p=p, q=q)
    with pytest.raises(AssertionError):
        SecondOrderNode2Vec(ei, 32, walk_length=3, context_size=4, p=2, q=0.5)


def test_generator_parser_still_yields_the_reference_defaults():
    from graphpope_amd.generate_node2vec_embedding import build_parser
    ns = vars(build_parser().parse_args([]))
    assert {k: ns[k] for k in ("embedding_dim", "walk_length", "context_size", "walks_per_node", "num_negative_samples", "p", "q",
                               "sparse")} == {"embedding_dim": 128, "walk_length": 20, "context_size": 10, "walks_per_node": 10,
                                              "num_negative_samples": 1, "p": 1, "q": 1, "sparse": True}
    ns = build_parser().parse_args("--p 0.25 --q 4".split())
    assert ns.p == 0.25 and ns.q == 4.0


# ---- the restatement on its own ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,seed", cases.FAN_RUNS)
def test_restatement_draws_the_node2vec_distribution_on_the_fan_graph(p, q, seed):
    """65 536 two-step walks from node 0.  Among those whose first step is 1, the second step's eight counts lie within 6 sigma of
    their binomial expectations (weights 0.25 : 1, 1, 1 : 2, 2, 2, 2 for (4, 0.5) and 4 : 1, 1, 1 : 0.5 x 4 for (0.25, 2)), and both
    the rejection tries and the exact pass took part."""
    rowptr, col = cases.canonical_csr(cases.fan_graph(), cases.N_FAN)
    pos, exact = cases.walks_biased_ref(rowptr, col, cases.N_FAN, np.zeros(cases.FAN_B, dtype=np.int64), 2, seed, p, q)
    assert (pos[:, 0] == 0).all() and np.isin(pos[:, 1], (1, 2, 3, 4)).all()
    assert (pos[np.isin(pos[:, 1], (2, 3, 4))][:, 2] == 0).all()                 # from 2..4 the only way is back
    first = np.bincount(pos[:, 1], minlength=5)[1:5]
    assert np.abs(first - cases.FAN_B / 4).max() <= 6 * np.sqrt(cases.FAN_B * 0.25 * 0.75)
    worst, m = cases.fan_second_step_deviation(pos, p, q)
    print(f"(p, q) = ({p}, {q}) seed {seed}: {m} walks through node 1, largest deviation {worst:.2f} sigma, exact pass {exact} times")
    assert worst <= 6.0
    assert 0 < exact < m // 2                                                    # both branches contribute


@pytest.fixture(scope="module")
def g70():
    ei = cases.graph70()
    rowptr, col = cases.canonical_csr(ei, cases.N70)
    return ei, rowptr, col, np.bincount(ei[0], minlength=cases.N70)


@pytest.mark.parametrize("p,q", cases.PQ70 + [(1.0, 1.0)])
def test_restatement_walks_the_70_node_graph(g70, p, q):
    ei, rowptr, col, deg = g70
    starts = cases.starts201()
    pos, exact = cases.walks_biased_ref(rowptr, col, cases.N70, starts, cases.L7, cases.SEED70, p, q)
    assert pos.shape == (201, cases.L7 + 1) and (pos[:, 0] == starts).all()
    edges = set(zip(ei[0].tolist(), ei[1].tolist()))
    for row in pos:
        for a, b in zip(row[:-1], row[1:]):
            assert (a, b) in edges or (a == b and deg[a] == 0), (a, b)
    for row in pos[(starts == 7) | (starts == 8)]:
        assert all(row[k + 1] == 15 - row[k] for k in range(cases.L7)), row       # 7, 8, 7, 8, ... whatever p says about returning
    assert (pos[starts == 1] == 1).all() and (pos[starts == 69] == 69).all()
    print(f"(p, q) = ({p}, {q}): exact pass {exact} times in {201 * cases.L7} steps")
    if (p, q) in ((0.25, 4.0), (1e6, 1.0), (1.0, 1e6)):
        assert exact > 0
    if (p, q) == (1.0, 1.0):
        assert exact == 0


def test_restatement_with_p_q_1_is_the_first_order_rule(g70):
    _, rowptr, col, _ = g70
    starts = cases.starts201()
    pos, exact = cases.walks_biased_ref(rowptr, col, cases.N70, starts, cases.L7, cases.SEED70, 1.0, 1.0)
    assert exact == 0 and np.array_equal(pos, cases.walks_first_order_ref(rowptr, col, cases.N70, starts, cases.L7, cases.SEED70))
    part, _ = cases.walks_biased_ref(rowptr, col, cases.N70, starts[50:100], cases.L7, cases.SEED70, 1.0, 1.0, first_row=50)
    assert np.array_equal(part, cases.walks_first_order_ref(rowptr, col, cases.N70, starts[50:100], cases.L7, cases.SEED70, first_row=50))


@pytest.mark.parametrize("p,q", [(0.25, 4.0), (1e6, 1.0)])
def test_restatement_rows_do_not_depend_on_the_call(g70, p, q):
    _, rowptr, col, _ = g70
    starts = cases.starts201()
    full, _ = cases.walks_biased_ref(rowptr, col, cases.N70, starts, cases.L7, cases.SEED70, p, q)
    part, _ = cases.walks_biased_ref(rowptr, col, cases.N70, starts[50:100], cases.L7, cases.SEED70, p, q, first_row=50)
    assert np.array_equal(part, full[50:100])
    other, _ = cases.walks_biased_ref(rowptr, col, cases.N70, starts, cases.L7, cases.SEED70 + 1, p, q)
    assert not np.array_equal(other, full)
