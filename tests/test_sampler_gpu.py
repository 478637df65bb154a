"""GPU fan-out sampler against its CPU restatement (bit for bit), against the properties NeighborSampler guarantees (a numpy
checker that shares no code with the sampler), on graphs constructed to put counts, degrees and repeats on the block,
fan-out and power-of-two edges of its kernels, and against the uniform distribution (chi-square, tests/sampler_uniformity.py)."""
import numpy as np
import pytest
import torch

import sampler_uniformity as su

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def graph():
    from graphpope_amd import engine, synth
    dev = engine.require_gpu()
    ei = synth.powerlaw_graph(6000, 40000, seed=7, alpha=0.9, shift=0.8)
    csr = engine.build_csr(torch.as_tensor(ei, device=dev), 6000)
    return dev, ei, csr


def _host_csr(csr):
    return csr.rowptr.cpu().numpy(), csr.col.cpu().numpy()[: csr.num_edges]


@pytest.mark.parametrize("sizes,seed", [((25, 10), 1), ((3,), 99), ((-1, 2), 5), ((1, 1, 1), 2**40 + 7)])
def test_matches_cpu_restatement_bit_for_bit(graph, oracle, sizes, seed):
    from graphpope_amd.sampler import NeighborSampler
    dev, _, csr = graph
    rowptr, col = _host_csr(csr)
    seeds = np.random.RandomState(3).choice(6000, 257, replace=False)
    n_id, adjs = NeighborSampler(csr.rowptr, csr.col, 6000, sizes).sample(torch.as_tensor(seeds, device=dev), seed=seed)
    want_n_id, want = np.asarray(seeds, np.int64), []
    for hop, size in enumerate(sizes):
        rp, cl, want_n_id = oracle.sample_hop(rowptr, col, want_n_id, size, seed, hop)
        want.append((rp, cl, len(want_n_id)))
    assert np.array_equal(n_id.cpu().numpy(), want_n_id)
    for adj, (rp, cl, n_src) in zip(adjs, want[::-1]):
        assert adj.n_src == n_src and np.array_equal(adj.rowptr.cpu().numpy(), rp) and np.array_equal(adj.col.cpu().numpy(), cl)


def test_neighbor_sampler_properties(graph):
    """What the reference relies on: targets first, destinations = first n_dst sources, samples are distinct true
    neighbours, rows with <= fan-out neighbours keep all of them, and the draw is roughly uniform."""
    from graphpope_amd.sampler import NeighborSampler
    dev, ei, csr = graph
    rowptr, col = _host_csr(csr)
    seeds = torch.arange(0, 1550, device=dev)
    sampler = NeighborSampler(csr.rowptr, csr.col, 6000, (25, 10))
    n_id, adjs = sampler.sample(seeds, seed=11)
    n_id = n_id.cpu().numpy()
    assert np.array_equal(n_id[:1550], np.arange(1550)) and len(np.unique(n_id)) == len(n_id)
    assert adjs[1].size(0) == 1550 and adjs[0].size(0) == adjs[1].size(1) and adjs[0].size(1) == len(n_id)
    for adj, fan in zip(adjs[::-1], (25, 10)):
        rp, cl = adj.rowptr.cpu().numpy(), adj.col.cpu().numpy()
        for i in range(0, adj.n_dst, 37):
            g = n_id[i]
            true = set(col[rowptr[g]:rowptr[g + 1]].tolist())
            got = n_id[cl[rp[i]:rp[i + 1]]]
            assert len(set(got.tolist())) == len(got) and set(got.tolist()) <= true
            assert len(got) == min(len(true), fan)
    # uniformity on the biggest hub: 400 draws of 10 out of d neighbours, every neighbour's frequency near 10/d
    hub = int(np.argmax(np.diff(rowptr)))
    d = int(rowptr[hub + 1] - rowptr[hub])
    counts = np.zeros(6000)
    for s in range(400):
        nid, (adj,) = NeighborSampler(csr.rowptr, csr.col, 6000, (10,)).sample(torch.tensor([hub], device=dev), seed=s)
        counts[nid.cpu().numpy()[1:]] += 1
    freq = counts[col[rowptr[hub]:rowptr[hub + 1]]] / 400
    q, dof = su.inclusion_chi_square(freq * 400, 400, 10)         # expected count 1.5 per neighbour, 2 647 of them
    print(f"hub of degree {d}: inclusion chi2 = {q:.1f} on {dof} dof, critical {su.critical(dof):.1f}")
    assert q < su.critical(dof) and freq.max() < 4 * 10 / d + 0.02


def test_sampled_batch_trains(graph):
    from graphpope_amd.sage import SAGE
    from graphpope_amd.sampler import NeighborSampler
    dev, _, csr = graph
    torch.manual_seed(0)
    feats = torch.randn(6000, 32, device=dev)
    labels = torch.randint(0, 4, (6000,), device=dev)
    model = SAGE(32, 4, 48, 2).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    sampler = NeighborSampler(csr.rowptr, csr.col, 6000, (25, 10))
    seeds = torch.arange(512, device=dev)
    first = last = None
    for step in range(25):
        n_id, adjs = sampler.sample(seeds, seed=step)
        loss = torch.nn.functional.cross_entropy(model(feats.index_select(0, n_id), adjs), labels[:512])
        opt.zero_grad(); loss.backward(); opt.step()
        first = loss.item() if first is None else first
        last = loss.item()
    assert last < 0.8 * first


# ----------------------------------------------------------------------------------------------------------------------
# Uniformity of the draw: one launch = 8 192 independent rows of the same degree
# ----------------------------------------------------------------------------------------------------------------------
N_HUBS = 8192


def _hub_picks(d, fanout, seed, n_hubs):
    """picks [n_hubs, fanout]: what one sample() call draws for n_hubs rows that all hold the leaves 0 .. d-1."""
    from graphpope_amd import engine
    from graphpope_amd.sampler import NeighborSampler
    dev = engine.require_gpu()
    n = d + n_hubs
    rowptr = np.concatenate([np.zeros(d, np.int64), np.arange(n_hubs + 1, dtype=np.int64) * d])
    col = np.tile(np.arange(d, dtype=np.int32), n_hubs)
    sampler = NeighborSampler(torch.as_tensor(rowptr, dtype=torch.int32, device=dev), torch.as_tensor(col, device=dev), n, (fanout,))
    n_id, (adj,) = sampler.sample(torch.arange(d, n, device=dev), seed=seed)
    n_id = n_id.cpu().numpy()
    assert np.array_equal(adj.rowptr.cpu().numpy(), np.arange(n_hubs + 1) * fanout)
    assert np.array_equal(n_id[:n_hubs], np.arange(d, n)) and len(n_id) <= n
    picks = n_id[adj.col.cpu().numpy()].reshape(n_hubs, fanout)          # leaf id = position in the row
    return picks


@pytest.mark.parametrize("seed", su.SEEDS)
@pytest.mark.parametrize("d,fanout", su.CASES)
def test_draw_is_uniform(d, fanout, seed):
    """Leaves 0 .. d-1, hubs d .. d+8191, every hub's row = the d leaves: one sample() call draws `fanout` of d neighbours
    8 192 times independently (the key mixes the node id).  Inclusion counts, slot 0 and -- for d <= 17 -- the ordered pair
    (slot 0, slot 1) must pass chi-square at an upper tail of 1e-4: the bound is the distribution's, the inputs are fixed."""
    su.assert_uniform(_hub_picks(d, fanout, seed, N_HUBS), d, f"d={d} f={fanout} seed={seed}")


@pytest.mark.parametrize("seed", su.SEEDS)
def test_ordered_pairs_are_uniform_on_a_full_feistel_domain(seed):
    """d = 64 fills the 6-bit domain (no cycle walk hides anything) and is the widest row with 3-bit halves.  The table above
    cannot see its pairs (8 192 rows over 4 032 cells); 2^18 rows put 65 in every cell.  A 4-round network gives a pair
    chi-square above 7 200 here, a 5-round one of 4 404-4 409, against a critical value of 4 373.5 on 4 031 degrees of freedom."""
    su.assert_uniform(_hub_picks(64, 2, seed, 1 << 18), 64, f"d=64 f=2 seed={seed} rows=2^18", pair=True)


# ----------------------------------------------------------------------------------------------------------------------
# Structure of one hop, checked without any of the sampler's code
# ----------------------------------------------------------------------------------------------------------------------
def _check_structure(rowptr, col, n, targets, fanout, out_rowptr, out_col, n_id):
    """Every row of one hop's output (host CSR rowptr / col over n nodes without repeated edges; out_col holds local ids)."""
    targets = np.asarray(targets, np.int64)
    t = len(targets)
    deg = (rowptr[targets + 1] - rowptr[targets]).astype(np.int64)
    keep = deg if fanout < 0 else np.minimum(deg, fanout)
    assert np.array_equal(out_rowptr, np.concatenate([[0], np.cumsum(keep)]))
    nnz = int(keep.sum())
    assert len(out_col) == nnz and np.array_equal(n_id[:t], targets)
    assert nnz == 0 or (out_col.min() >= 0 and out_col.max() < len(n_id))
    g = n_id[out_col]
    row = np.repeat(np.arange(t), keep)                                       # output row of every slot
    assert len(np.unique(row * n + g)) == nnz, "a row repeats a neighbour"
    edges = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr)) * n + col[: rowptr[-1]]
    assert np.isin(targets[row] * n + g, edges).all(), "a pick is no neighbour of its target"
    whole = (deg <= fanout) if fanout >= 0 else np.ones(t, bool)
    src = rowptr[targets[row]] + np.arange(nnz) - np.asarray(out_rowptr, np.int64)[row]       # CSR position if the row is kept whole
    assert np.array_equal(g[whole[row]], col[src[whole[row]]]), "a row within the fan-out is not the CSR row in order"
    seq = np.concatenate([targets, g])
    uniq, first = np.unique(seq, return_index=True)
    want_n_id = uniq[np.argsort(first)]                                       # first appearances, in order
    assert np.array_equal(n_id, want_n_id)
    pos = np.full(n, -1, np.int64)
    pos[want_n_id] = np.arange(len(want_n_id))
    assert np.array_equal(out_col, pos[g])


def _check_batch(oracle, rowptr, col, n, seeds, sizes, seed, n_id, adjs):
    """A host-sized batch, hop by hop: the structure checker on every row, and the CPU restatement bit for bit."""
    n_id = n_id.cpu().numpy()
    targets = np.asarray(seeds, np.int64)
    assert len(adjs) == len(sizes)
    for hop, (fanout, adj) in enumerate(zip(sizes, adjs[::-1])):
        rp, cl = adj.rowptr.cpu().numpy(), adj.col.cpu().numpy()
        assert adj.n_dst == len(targets) and adj.n_src <= len(n_id)
        ids = n_id[: adj.n_src]
        _check_structure(rowptr, col, n, targets, fanout, rp, cl, ids)
        want_rp, want_cl, want_ids = oracle.sample_hop(rowptr, col, targets, fanout, seed, hop)
        assert np.array_equal(rp, want_rp) and np.array_equal(cl, want_cl) and np.array_equal(ids, want_ids)
        targets = ids
    assert len(targets) == len(n_id)


def _check_device_batch(batch, n_id, adjs):
    """A DeviceBatch against the host-sized batch of the same draw: dims rows {n_dst, n_src, nnz, 0}, the valid prefixes equal,
    every row pointer from n_dst to the capacity = nnz."""
    dims = batch.dims.cpu().numpy()
    for hop, (got, want) in enumerate(zip(batch.adjs[::-1], adjs[::-1])):
        nnz = want.col.numel()
        assert dims[hop].tolist() == [want.n_dst, want.n_src, nnz, 0]
        rp = got.rowptr.cpu().numpy()
        assert np.array_equal(rp[: want.n_dst + 1], want.rowptr.cpu().numpy()) and (rp[want.n_dst:] == nnz).all()
        assert torch.equal(got.col[:nnz], want.col)
        assert torch.equal(batch.n_ids[hop][: want.n_src], n_id[: want.n_src])
    assert torch.equal(batch.n_id[: n_id.numel()], n_id)


def _device_graph(rowptr, col, dev):
    col_dev = torch.zeros(max(len(col), 1), dtype=torch.int32, device=dev)        # a graph without edges still needs an address
    col_dev[: len(col)] = torch.as_tensor(col, dtype=torch.int32)
    return torch.as_tensor(rowptr, dtype=torch.int32, device=dev), col_dev


def _run_both_forms(oracle, sampler, batch, rowptr, col, n, seeds, seed):
    """sample() checked against the structure checker and the restatement; with positive fan-outs also sample_device() into
    `batch` (made here if None), filled twice, against sample()'s result.  Returns the batch."""
    from graphpope_amd.sampler import DeviceBatch
    dev = sampler.rowptr.device
    seeds_dev = torch.as_tensor(np.asarray(seeds, np.int64), device=dev)
    n_id, adjs = sampler.sample(seeds_dev, seed=seed)
    _check_batch(oracle, rowptr, col, n, seeds, sampler.sizes, seed, n_id, adjs)
    if all(f > 0 for f in sampler.sizes):
        batch = batch or DeviceBatch(len(seeds), sampler.sizes, dev)
        for _ in range(2):
            assert sampler.sample_device(seeds_dev, seed=seed, out=batch) is batch
            _check_device_batch(batch, n_id, adjs)
    return batch


# ----------------------------------------------------------------------------------------------------------------------
# Constructed graphs.  CHAIN = items per block of the two chained scans (sampler.hip: CHAIN_ITEMS)
# ----------------------------------------------------------------------------------------------------------------------
CHAIN = 1024


def _from_rows(rows, n):
    """CSR of {node: neighbour list}."""
    deg = np.zeros(n, np.int64)
    for g, r in rows.items():
        deg[g] = len(r)
    col = np.concatenate([np.asarray(rows[g], np.int64) for g in sorted(rows)] + [np.zeros(0, np.int64)])
    return np.concatenate([[0], np.cumsum(deg)]), col


def _ring3(n):
    """Every node i has the three neighbours i+1, i+2, i+5 (mod n), n >= 6."""
    return np.arange(n + 1, dtype=np.int64) * 3, ((np.arange(n)[:, None] + np.array([1, 2, 5])) % n).ravel()


def _ring3_seeds(t):
    return _ring3(4100) + (4100, np.random.RandomState(1).permutation(4100)[:t])


def _few_edges(nnz):
    """1 500 targets of degree 0 or 1, `nnz` of them with a neighbour: a new node (even targets) or another target (odd)."""
    rows = {int(i): [1500 + int(i) if i % 2 == 0 else (int(i) + 1) % 1500] for i in np.random.RandomState(2).permutation(1500)[:nnz]}
    return _from_rows(rows, 3000) + (3000, np.arange(1500))


def _hub_and_leaves(first_slot):
    """2 000 targets with two neighbours each, one of them the same hub, so the hub's rank is read in every rank block.
    first_slot 0: every row is {hub, own leaf}; 1023: the hub first appears in the last slot of block 0 and next in slot 1024."""
    hub, rows = 4000, {}
    for i in range(2000):
        if first_slot == 0 or i >= 512:
            rows[i] = [hub, 2000 + i]
        elif i == 511:
            rows[i] = [2000 + i, hub]
        else:
            rows[i] = [2000 + i, 4001 + i]
    rp, cl = _from_rows(rows, 4600)
    assert int(np.flatnonzero(cl == hub)[0]) == first_slot and (first_slot == 0 or cl[1024] == hub)
    return rp, cl, 4600, np.arange(2000)


def _degree_edges():
    """Targets 5000.. whose degrees sit at f-1, f, f+1 for the fan-outs 1, 2, 10, 25 and at 2^k-1, 2^k, 2^k+1 for k = 2..12
    (the Feistel width changes above every power of two; 2^k + 1 with even k walks the longest cycle), over a pool of 5 000."""
    degs = [f + e for f in (1, 2, 10, 25) for e in (-1, 0, 1)] + [(1 << k) + e for k in range(2, 13) for e in (-1, 0, 1)]
    rng = np.random.RandomState(4)
    rows = {5000 + i: rng.choice(5000, dg, replace=False) for i, dg in enumerate(degs)}
    return _from_rows(rows, 5000 + len(degs)) + (5000 + len(degs), 5000 + rng.permutation(len(degs)))


def _big_row():
    """Node 0 has 3 000 neighbours (more than a block's 256 threads, more than one rank block); a third of them lead on to node
    0 and a new node, a third to the next one, a third nowhere; node 6500 is isolated."""
    rows = {0: list(range(1, 3001))}
    for i in range(1, 3001):
        if i % 3 == 0:
            rows[i] = [0, 3000 + i]
        elif i % 3 == 1:
            rows[i] = [i % 3000 + 1]
    return _from_rows(rows, 6600) + (6600, np.array([6500, 0, 5, 6501]))


def _complete(n):
    return _from_rows({i: [j for j in range(n) if j != i] for i in range(n)}, n) + (n, np.arange(n))


def _isolated():
    return np.zeros(301, np.int64), np.zeros(0, np.int64), 300, np.arange(0, 200, 2)


def _constructed_cases():
    cases = {}
    for t in (1, CHAIN - 1, CHAIN, CHAIN + 1, 2 * CHAIN - 1, 2 * CHAIN, 2 * CHAIN + 1):      # count scan: entry T of the row pointer
        cases[f"count_scan_T{t}_sampled"] = (lambda t=t: _ring3_seeds(t), (2,))
        cases[f"count_scan_T{t}_whole_rows"] = (lambda t=t: _ring3_seeds(t), (3,))
    cases["rank_scan_nnz_is_cap_1024x1"] = (lambda: _ring3_seeds(1024), (1,))                # slot nnz = cap opens a block of its own
    cases["rank_scan_nnz_is_cap_512x2"] = (lambda: _ring3_seeds(512), (2,))
    for nnz in (0, 1, CHAIN - 1, CHAIN, CHAIN + 1):                                          # nnz far below cap = 37 500
        cases[f"rank_scan_nnz{nnz}"] = (lambda nnz=nnz: _few_edges(nnz), (25,))
    cases["no_edges_two_hops"] = (_isolated, (25, 10))                                       # hop 1: 100 true targets, capacity 2 600
    cases["hub_first_in_slot_0"] = (lambda: _hub_and_leaves(0), (25,))
    cases["hub_first_in_slot_1023"] = (lambda: _hub_and_leaves(1023), (25,))
    cases["ring_among_seeds_sampled"] = (lambda: _ring3(2500) + (2500, np.arange(2500)), (2,))   # every pick is a target, every block
    cases["ring_among_seeds_whole_rows"] = (lambda: _ring3(2500) + (2500, np.arange(2500)), (3,))
    for f in (1, 2, 10, 25):
        cases[f"degree_edges_f{f}"] = (_degree_edges, (f,))
    cases["all_neighbours_one_hop"] = (_big_row, (-1,))
    cases["all_neighbours_two_hops"] = (_big_row, (-1, -1))
    for n in (1, 2, 3):                                                                      # the position-key map is all tail
        cases[f"complete_graph_N{n}"] = (lambda n=n: _complete(n), (1, 1))
    cases["five_hops_regions_alternate"] = (lambda: _ring3_seeds(16), (2, 2, 2, 2, 2))
    return cases


CONSTRUCTED = _constructed_cases()


@pytest.mark.parametrize("name", list(CONSTRUCTED))
def test_constructed_case(name, oracle):
    """Counts, degrees and repeats placed exactly on the edges of the kernels: host-sized and device-extent form, every row
    through the structure checker, every hop against the CPU restatement bit for bit."""
    from graphpope_amd import engine
    from graphpope_amd.sampler import NeighborSampler
    dev = engine.require_gpu()
    make, sizes = CONSTRUCTED[name]
    rowptr, col, n, seeds = make()
    sampler = NeighborSampler(*_device_graph(rowptr, col, dev), n, sizes)
    _run_both_forms(oracle, sampler, None, rowptr, col, n, seeds, seed=7)


@pytest.mark.parametrize("sizes", [(4,), (4, 4)])                 # node 0 has at most 4 neighbours: its row is kept whole
@pytest.mark.parametrize("n", [5, 6, 7, 1025, 1026, 1027])
def test_tail_of_the_position_key_map_is_cleared(n, sizes, oracle):
    """The map is cleared four keys at a time and its last N & 3 keys by a tail.  Those nodes are seeds of call 1 (their keys
    mark them as targets) and neighbours of node 0, which call 2 seeds on the same sampler and the same DeviceBatch: a key left
    over from call 1 would relabel them as targets.  (A DeviceBatch holds a fixed number of seeds: call 2 seeds nodes 0, 1, 2.)"""
    from graphpope_amd import engine
    from graphpope_amd.sampler import NeighborSampler
    dev = engine.require_gpu()
    tail = list(range(n - (n & 3), n))
    rows = {i: [i + 1 if i + 1 < n else 1] for i in range(1, n)}
    rows[0] = tail + [1]
    rowptr, col = _from_rows(rows, n)
    sampler = NeighborSampler(*_device_graph(rowptr, col, dev), n, sizes)
    batch = _run_both_forms(oracle, sampler, None, rowptr, col, n, tail, seed=3)
    assert _run_both_forms(oracle, sampler, batch, rowptr, col, n, [0, 1, 2][: len(tail)], seed=3) is batch


def test_seed_words_wrap(graph):
    """The host word and the device word add up modulo 2^64: (2^64 - 1) + 5 draws what seed 4 draws."""
    from graphpope_amd.sampler import NeighborSampler
    dev, _, csr = graph
    seeds = torch.arange(300, 557, device=dev)
    sampler = NeighborSampler(csr.rowptr, csr.col, 6000, (25, 10))
    n_id, adjs = sampler.sample(seeds, seed=4)
    other = sampler.sample(seeds, seed=5)[0]
    assert other.numel() != n_id.numel() or not torch.equal(other, n_id)                     # the seed matters at all
    batch = sampler.sample_device(seeds, seed=2**64 - 1, seed_dev=torch.tensor([5], dtype=torch.int64, device=dev))
    _check_device_batch(batch, n_id, adjs)
