"""Deterministic mode on the device (sage_set_deterministic, include/graphpope_hip.h): the fixed-order sum behind
sage_scatter_mean_det bit for bit against the NumPy restatement of its contract, the whole backward pass on every kernel path, and
what the mode is for -- a model, a training step (eager and replayed), the evaluation metrics and the command line give the same
bits twice.  Every test that turns the switch on does so through the `det` fixture or a with block, which turn it off again."""
import ctypes

import numpy as np
import pytest
import torch

import deterministic_cases as det_cases
import sage_backward_cases as cases
from sage_backward_cases import SENTINEL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from graphpope_amd import engine
    return engine.require_gpu()


@pytest.fixture(scope="module")
def lib():
    from graphpope_amd import _lib
    return _lib.load()


@pytest.fixture
def det(lib):
    assert lib.sage_get_deterministic() == 0, "an earlier test left the switch on"
    lib.sage_set_deterministic(1)
    yield
    lib.sage_set_deterministic(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _run_sum(lib, dev, rowptr, col, n_src, n_dst, gagg, gx, scratch=None, dims=None, nnz=None):
    """sage_scatter_mean_det on device copies of the arguments (or on the device tensors given); returns grad_x as NumPy."""
    from graphpope_amd import _lib
    t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rowptr, col, gagg, gx = t(rowptr), t(col), t(gagg), t(gx)
    nnz = int(col.numel()) if nnz is None else nnz
    c = gagg.shape[1]
    need = lib.sage_scatter_mean_det_scratch_bytes(n_src, n_dst, nnz)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    assert scratch.numel() >= need
    _lib.check(lib.sage_scatter_mean_det(_lib.ptr(rowptr), _lib.ptr(col), n_src, n_dst, nnz, _lib.ptr(gagg), c, _lib.ptr(gx), _lib.ptr(scratch),
                                         scratch.numel(), _lib.ptr(dims), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return gx.cpu().numpy()


@pytest.fixture(scope="module")
def block():
    return det_cases.hand_built_block()


def _inputs(c, n_dst, n_src, seed):
    """randn gradients; grad_x on entry: randn below n_dst, the sentinel behind (those rows must be overwritten, not added to)."""
    rs = np.random.RandomState(seed)
    gagg = rs.randn(n_dst, c).astype(np.float32)
    gx = np.full((n_src, c), SENTINEL, dtype=np.float32)
    gx[:n_dst] = rs.randn(n_dst, c)
    return gagg, gx


@pytest.mark.parametrize("c", [256, 260, 37, 4], ids=["full_slab", "ragged_second_slab", "scalar", "one_16_byte_unit"])
def test_the_sum_equals_its_contract_bit_for_bit(block, c, dev, lib):
    """A block of 130 destinations and 200 sources with lists of 0, 1, 2 (one destination twice), 64, 65 and 129 entries, below and behind
    the destinations: every bit of grad_x equals the float32 loop of the contract (product rounded, added in ascending slot order)."""
    rowptr, col = block
    gagg, gx = _inputs(c, det_cases.N_DST, det_cases.N_SRC, seed=c)
    want = det_cases.scatter_mean_reference(rowptr, col, det_cases.N_SRC, det_cases.N_DST, gagg, gx)
    got = _run_sum(lib, dev, rowptr, col, det_cases.N_SRC, det_cases.N_DST, gagg, gx)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, "%d elements differ, the first at %s: got %r, want %r" % (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    assert (got[det_cases.IN0_HIGH] == 0).all() and not np.signbit(got[det_cases.IN0_HIGH]).any()      # never listed, behind the destinations: +0
    assert np.array_equal(_bits(got[det_cases.IN0_LOW]), _bits(gx[det_cases.IN0_LOW]))                   # never listed, a destination: as found


@pytest.mark.parametrize("c", [4, 37])
def test_the_index_scan_carries_over_its_rounds(c, dev, lib):
    """2 x 8192 + 3 sources, so the one-block scan of the index takes three rounds: lists only at sources 0, 8191 | 8192, 16383 | 16384
    and 16386, the one at 8192 with 70 entries.  Where a list behind a round edge begins, and where its sorted copy goes, is the carry of
    the rounds before: every bit of grad_x equals the contract, and the unlisted rows behind the destinations are +0."""
    n_dst, n_src = det_cases.CARRY_N_DST, det_cases.CARRY_N_SRC
    rowptr, col = det_cases.scan_carry_block()
    gagg, gx = _inputs(c, n_dst, n_src, seed=c)
    want = det_cases.scatter_mean_reference(rowptr, col, n_src, n_dst, gagg, gx)
    got = _run_sum(lib, dev, rowptr, col, n_src, n_dst, gagg, gx)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, "%d elements differ, the first at %s: got %r, want %r" % (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    unlisted = np.setdiff1d(np.arange(n_dst, n_src), list(det_cases.CARRY_LISTS))
    assert len(unlisted) == n_src - n_dst - 5 and (_bits(got[unlisted]) == 0).all()                      # +0, not the sentinel and not -0


@pytest.mark.parametrize("c", [256, 37])
def test_the_order_inside_a_destination_row_does_not_matter(block, c, dev, lib):
    """col permuted inside every destination row: the same bits, because a list is ordered by destination and equal destinations add
    equal terms."""
    rowptr, col = block
    gagg, gx = _inputs(c, det_cases.N_DST, det_cases.N_SRC, seed=c + 1)
    first = _run_sum(lib, dev, rowptr, col, det_cases.N_SRC, det_cases.N_DST, gagg, gx)
    rs = np.random.RandomState(9)
    for trial in range(2):
        perm = col.copy()
        for i in range(det_cases.N_DST):
            rs.shuffle(perm[rowptr[i]:rowptr[i + 1]])
        assert not np.array_equal(perm, col)
        again = _run_sum(lib, dev, rowptr, perm, det_cases.N_SRC, det_cases.N_DST, gagg, gx)
        assert np.array_equal(_bits(again), _bits(first)), trial


@pytest.mark.parametrize("c", [256, 37])
def test_device_extents_read_and_write_the_true_rows_only(c, dev, lib):
    """Buffers and scratch at the capacity (130, 200), `dims` on the device, true sizes (100, 170) and then (40, 90) on the SAME buffers
    and scratch: the true prefix equals the host-sized call and the contract bit for bit, the rows past the true sources keep their
    sentinel, and neither the NaN rows past the true destinations, nor the indices past the true slots (which point at rows that must
    stay untouched), nor the larger run's index leave a trace."""
    n_dst_cap, n_src_cap = det_cases.N_DST, det_cases.N_SRC
    blocks = [(n, m, det_cases.random_block(n, m, seed=n)) for n, m in ((100, 170), (40, 90))]
    nnz_cap = max(len(col) for _, _, (_, col) in blocks) + 64
    scratch = torch.empty(lib.sage_scatter_mean_det_scratch_bytes(n_src_cap, n_dst_cap, nnz_cap), dtype=torch.uint8, device=dev)
    rowptr_d = torch.empty(n_dst_cap + 1, dtype=torch.int32, device=dev)
    col_d = torch.empty(nnz_cap, dtype=torch.int32, device=dev)
    gagg_d, gx_d = torch.empty(n_dst_cap, c, device=dev), torch.empty(n_src_cap, c, device=dev)
    dims_d = torch.zeros(4, dtype=torch.int32, device=dev)
    for n_dst, n_src, (rowptr, col) in blocks:
        assert np.bincount(col, minlength=n_src).max() > 64
        gagg, gx = _inputs(c, n_dst, n_src, seed=n_dst + c)
        gx[n_dst:] = SENTINEL
        want = det_cases.scatter_mean_reference(rowptr, col, n_src, n_dst, gagg, gx)
        host_sized = _run_sum(lib, dev, rowptr, col, n_src, n_dst, gagg, gx.copy())
        assert np.array_equal(_bits(host_sized), _bits(want))
        rp, cl = cases.padded_csr(rowptr, col, n_dst_cap, nnz_cap, n_src, n_src_cap, np.random.RandomState(n_dst))
        rowptr_d.copy_(torch.from_numpy(rp))
        col_d.copy_(torch.from_numpy(cl))
        gagg_d.copy_(torch.from_numpy(cases.nan_padded(gagg, n_dst_cap)))
        full = np.full((n_src_cap, c), SENTINEL, dtype=np.float32)
        full[:n_dst] = gx[:n_dst]
        gx_d.copy_(torch.from_numpy(full))
        dims_d.copy_(torch.tensor([n_dst, n_src, len(col), 0], dtype=torch.int32))
        got = _run_sum(lib, dev, rowptr_d, col_d, n_src_cap, n_dst_cap, gagg_d, gx_d, scratch=scratch, dims=dims_d, nnz=nnz_cap)
        assert not np.isnan(got).any(), (n_dst, "NaN from the padding")
        assert np.array_equal(_bits(got[:n_src]), _bits(host_sized)), (n_dst, int((_bits(got[:n_src]) != _bits(host_sized)).sum()))
        assert np.array_equal(got[n_src:], np.full_like(got[n_src:], SENTINEL)), (n_dst, "rows past the true sources were written")


# ---- the whole backward pass, switch on -----------------------------------------------------------------------------------------
_BACKWARD = [cases._case(shape, extra, family=family) for shape in ((1030, 40, 24), (515, 37, 30), (4160, 256, 256)) for extra in (0, 300)
             for family in ("exact", "rounding")]
_BACKWARD += [cases._case((1030, 40, 24), extra, trues=(999, 300)) for extra in (0, 300)]


@pytest.mark.parametrize("case", _BACKWARD, ids=[c["id"] for c in _BACKWARD])
def test_backward_on_every_path_with_the_switch_on(case, det, dev, lib):
    """sage_conv_backward in deterministic mode on the dual, the split-K twin and the stream-K path, host-sized and with device extents
    (two true sizes on the same buffers and scratch): the exact family equals the exact sums, the rounding family stays within
    Reference.bounds -- derived for any order of the additions, so the fixed order needs no other bound -- and a second call on the same
    inputs gives the same bits in all four gradients."""
    import test_sage_backward_gpu as bwd
    name = bwd._backward_name(lib, case, dev)
    assert "k_scatter_sum_det" in name and "k_scatter_mean" not in name and "k_scatter_and_finals" not in name and "k_zero_rows" not in name
    cap = case["shape"][0]
    trues = case["trues"] or (cap,)
    refs = [cases.reference(case, n) for n in trues]
    buffers = bwd.Buffers(case, dev, max(r.nnz for r in refs) + (64 if case["trues"] else 0))     # (scratch sized under the mode)
    outs = lambda: [t.clone() for t in (buffers.grad_x, buffers.grad_w_l, buffers.grad_w_r, buffers.grad_b)]
    for ref in refs:
        buffers.load(ref, extents=case["trues"] is not None)
        bwd._check(case, ref, buffers.run(lib), "true %d of %d" % (ref.n, cap))
        first = outs()
        buffers.run(lib)
        for a, b in zip(first, outs()):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- what the mode is for: the same bits twice ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph(dev):
    from graphpope_amd import engine, synth
    ei = synth.powerlaw_graph(6000, 40000, seed=7, alpha=0.9, shift=0.8)
    return engine.build_csr(torch.as_tensor(ei, device=dev), 6000)


def test_model_gradients_are_the_same_bits_twice(graph, det, dev):
    """A 2-hop SAGE (40 -> 48 -> 5, dropout 0.5 under a fixed seed) on one sampled batch of 512 seeds, forward and backward twice."""
    from graphpope_amd.sage import SAGE, cross_entropy
    from graphpope_amd.sampler import NeighborSampler
    feats = torch.randn(6000, 40, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    seeds = torch.arange(100, 612, device=dev)
    y = torch.randint(0, 5, (512,), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    n_id, adjs = NeighborSampler(graph.rowptr, graph.col, 6000, (25, 10)).sample(seeds, seed=5)
    x = feats[n_id]
    torch.manual_seed(0)
    m = SAGE(40, 5, 48, 2, dropout=0.5).to(dev)
    m.train(True)
    grads = []
    for _ in range(2):
        torch.manual_seed(123)                                     # the dropout seed is drawn from torch's generator
        for p in m.parameters():
            p.grad = None
        cross_entropy(m(x, adjs), y).backward()
        grads.append([p.grad.clone() for p in m.parameters()])
    assert len(grads[0]) == 8 and bool(grads[0][0].abs().sum() > 0) and bool(grads[0][2].abs().sum() > 0)
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def _train(graph, dev, use_graph, state, steps=8):
    from graphpope_amd.optim import Adam
    from graphpope_amd.sage import SAGE
    from graphpope_amd.sampler import NeighborSampler
    from graphpope_amd.train import SageTrainStep
    feats = torch.randn(6000, 40, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    labels = torch.randint(0, 5, (6000,), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    perm = torch.randperm(6000, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    sampler = NeighborSampler(graph.rowptr, graph.col, 6000, (25, 10))
    m = SAGE(40, 5, 48, 3).to(dev)
    m.load_state_dict(state)
    opt = Adam(m.parameters(), lr=0.01, max_grad_norm=0.5)
    st = SageTrainStep(m, opt, feats, 256, (25, 10), sampler=sampler, clip=None, graph=use_graph, seed=11)
    losses = []
    for i in range(steps):
        sd = perm[(i % 6) * 256:(i % 6 + 1) * 256].contiguous()
        losses.append(st.step(sd, labels[sd].contiguous()).item())
    torch.cuda.synchronize()
    tensors = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return losses, tensors, st.deterministic


@pytest.fixture(scope="module")
def start_state(dev):
    from graphpope_amd.sage import SAGE
    torch.manual_seed(0)
    return {k: v.clone() for k, v in SAGE(40, 5, 48, 3).to(dev).state_dict().items()}


def _same(a, b, what):
    (la, ta, _), (lb, tb, _) = a, b
    assert la == lb, (what, "losses", la, lb)
    assert ta.keys() == tb.keys() and any("running_var" in k for k in ta)
    for k in ta:                                                    # every parameter and every BatchNorm running statistic
        assert torch.equal(ta[k], tb[k]), (what, "the first tensor that differs", k, float((ta[k].float() - tb[k].float()).abs().max()))


def test_training_step_is_a_function_of_its_inputs(graph, start_state, det, dev):
    """8 steps of SageTrainStep (sampler inside the step, Adam with the clip inside) from the same state_dict: eager twice, replayed
    twice, and eager against replayed -- equal losses as floats, every parameter and running statistic torch.equal."""
    eager = [_train(graph, dev, False, start_state) for _ in range(2)]
    assert eager[0][2] is True and eager[0][0][-1] < eager[0][0][0]
    _same(eager[0], eager[1], "eager twice")
    replayed = [_train(graph, dev, True, start_state) for _ in range(2)]
    _same(replayed[0], replayed[1], "replayed twice")
    _same(eager[0], replayed[0], "eager against replayed")


def test_training_step_with_the_switch_off_is_what_it_was(graph, start_state, lib, dev):
    """The same body with the mode off meets the bounds of test_train_gpu.py::test_replayed_step_equals_the_eager_step: the mode
    changes nothing else."""
    assert lib.sage_get_deterministic() == 0
    (la, ta, da), (lb, tb, _) = _train(graph, dev, False, start_state), _train(graph, dev, True, start_state)
    assert da is False
    assert np.allclose(la, lb, rtol=1e-4) and la[-1] < la[0]
    for k in ta:
        if ta[k].is_floating_point() and "running" not in k:
            assert float((ta[k] - tb[k]).norm()) <= 0.1 * float(ta[k].norm()) + 1e-6, k


@pytest.mark.parametrize("m,c", [(1550, 7), (5000, 300), (700, 600)], ids=["registers_1", "registers_8", "three_passes"])
def test_metrics_are_the_same_bits_twice(m, c, lib, dev):
    """EvalMetrics.update in deterministic mode (one block, one add per launch): two fresh accumulators read back the same loss-sum bits
    and counts; against the default mode the counts are equal and the float64 loss sum agrees to 1e-12 (at most 5 000 terms)."""
    from graphpope_amd import sage
    logits = torch.randn(m, c, device=dev, generator=torch.Generator(device=dev).manual_seed(m))
    y = torch.randint(0, c, (m,), device=dev, generator=torch.Generator(device=dev).manual_seed(c))
    y[::17] = -100

    def words():
        acc = sage.EvalMetrics(dev)
        acc.update(logits, y)
        acc.update(logits[: m // 2], y[: m // 2])
        return acc.acc.cpu().numpy().copy()

    off = words()
    with sage.deterministic():
        on = [words(), words()]
    assert not sage.is_deterministic()
    assert np.array_equal(on[0], on[1])
    assert np.array_equal(on[0][1:], off[1:]) and on[0][2] == (m - len(range(0, m, 17))) + (m // 2 - len(range(0, m // 2, 17)))
    loss_on, loss_off = float(on[0][:1].view(np.float64)[0]), float(off[:1].view(np.float64)[0])
    assert loss_on > 0 and abs(loss_on - loss_off) <= 1e-12 * abs(loss_off)


def test_command_line_with_a_seed_ends_the_same_twice(capsys, monkeypatch, tmp_path, lib, dev):
    """GRAPHPOPE_DETERMINISTIC=1 python -m graphpope_amd.main on a 3 000-node graph, twice: the same epoch lines and test accuracy, and
    the switch is off again afterwards."""
    from graphpope_amd import main as cli, synth, utils as gp
    n = 3000
    rs = np.random.RandomState(4)
    ei = synth.powerlaw_graph(n, 20000, seed=3, alpha=0.9, shift=0.8)
    split = rs.rand(n)
    np.savez(tmp_path / "pubmed.npz", x=rs.rand(n, 500).astype(np.float32), y=rs.randint(0, 3, size=n), edge_index=np.asarray(ei),
             train_mask=split < 0.5, val_mask=(split >= 0.5) & (split < 0.75), test_mask=split >= 0.75)
    monkeypatch.setenv("GRAPHPOPE_DATA_DIR", str(tmp_path))
    monkeypatch.setenv("GRAPHPOPE_DETERMINISTIC", "1")
    runs = []
    for _ in range(2):
        gp.clear_cache()
        capsys.readouterr()
        acc = cli.main(["--dataset", "pubmed", "--embedding_space", "geodesic", "--sampling_method", "stochastic", "--num_anchor_nodes", "8",
                        "--num_layers", "2", "--batch_size", "256", "--epochs", "2"])
        lines = [line for line in capsys.readouterr().out.splitlines() if line.startswith(("epoch ", "test_acc"))]
        runs.append((acc, lines))
        assert lib.sage_get_deterministic() == 0
    gp.clear_cache()
    assert len(runs[0][1]) == 3 and runs[0] == runs[1], runs
