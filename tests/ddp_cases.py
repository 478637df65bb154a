"""Builders and restatements shared by tests/test_ddp_cpu.py and tests/test_ddp_gpu.py (data-parallel SAGE training,
graphpope_amd.parallel and csrc/grad_bucket.hip).  Not a test module; importable without a GPU."""
import numpy as np
import torch

# ------------------------------------------------------------------------------------------------ partition
PARTITION_N = (1, 2, 5, 6, 7, 31, 1551)
PARTITION_WORLD = (1, 2, 3, 8)


def sampler_indices(n, world, rank, shuffle, seed, epoch):
    """What Lightning's loader of rank `rank` iterates over: torch's DistributedSampler itself."""
    from torch.utils.data import DistributedSampler
    s = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed, drop_last=False)
    s.set_epoch(epoch)
    return list(s)


# ------------------------------------------------------------------------------------------------ bucket layout and pack
LAYOUT_LISTS = ([0, 1, 3, 4, 5], [5, 4, 3, 1, 0], [1], [0], [0, 0, 7, 0], [4, 4, 4], [3, 3, 3], [255, 256, 257, 4096, 4097], [])
SCALES = (1.0, 0.5, 1.0 / 3.0, 0.125)
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)


def layout_restatement(numel):
    """(offsets, total) in NumPy: every tensor starts where the one before ended, rounded up to 4 elements."""
    numel = np.asarray(numel, dtype=np.int64)
    padded = (numel + 3) // 4 * 4
    ends = np.cumsum(padded)
    return (ends - padded).tolist(), int(ends[-1]) if numel.size else 0


def pack_sizes(chunk):
    """One list with every size of the issue: the small ones, the 16-byte and block-size edges, and the per-block chunk +- 1."""
    return [0, 1, 3, 4, 5, 255, 256, 257, chunk - 1, chunk, chunk + 1]


def gradient_values(n, seed):
    """float32 [n]: normal floats over twelve binades (far from the denormals, also after * 0.125) with NaN, +-inf and +-0 sprinkled in
    where there is room -- always including the last element, next to the padding."""
    rng = np.random.RandomState(seed)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    g[g == 0] = 1.0
    if n >= 8:
        at = rng.choice(n - 1, SPECIALS.size, replace=False)
        g[at] = SPECIALS
        g[n - 1] = SPECIALS[seed % SPECIALS.size]
    elif n >= 1:
        g[n - 1] = SPECIALS[seed % SPECIALS.size]
    return g


def pack_expected(grads, scale):
    """The bucket sage_grad_bucket_pack must leave, as uint32 bits: np.float32(g) * np.float32(scale), one rounding; padding +0.0."""
    offsets, total = layout_restatement([g.size for g in grads])
    flat = np.zeros(total, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for o, g in zip(offsets, grads):
            flat[o:o + g.size] = g.astype(np.float32) * np.float32(scale)
    return flat.view(np.uint32)


# ------------------------------------------------------------------------------------------------ the two-rank model
NODES, EDGES, C_IN, HIDDEN, CLASSES, BATCH, FANOUT, LAYERS = 400, 2400, 12, 8, 3, 16, (3, 2), 3
LR, MAX_NORM, BETAS, EPS = 0.01, 0.5, (0.9, 0.999), 1e-8
STEP_SEED = 11


def make_model(dev):
    """The reference's default depth (num_layers = 3 over two hops: the third conv never runs), dropout 0.5."""
    from graphpope_amd.sage import SAGE
    torch.manual_seed(0)
    return SAGE(C_IN, CLASSES, HIDDEN, LAYERS).to(dev)


def make_data(dev, n_batches):
    """(feats, pool): float32 [NODES, C_IN] features and n_batches pre-sampled batches (DeviceBatch, labels) of BATCH seeds, the same on
    every rank that calls it."""
    from graphpope_amd import engine, synth
    from graphpope_amd.sampler import DeviceBatch, NeighborSampler
    ei = synth.powerlaw_graph(NODES, EDGES, seed=7, alpha=0.9, shift=0.8)
    csr = engine.build_csr(torch.as_tensor(ei, device=dev), NODES)
    feats = torch.randn(NODES, C_IN, generator=torch.Generator().manual_seed(1)).to(dev)
    labels = torch.randint(0, CLASSES, (NODES,), generator=torch.Generator().manual_seed(2)).to(dev)
    perm = torch.randperm(NODES, generator=torch.Generator().manual_seed(3)).to(dev)
    sampler = NeighborSampler(csr.rowptr, csr.col, NODES, FANOUT)
    pool = []
    for i in range(n_batches):
        sd = perm[i * BATCH:(i + 1) * BATCH].contiguous()
        n_id, adjs = sampler.sample(sd, seed=i)
        db = DeviceBatch(BATCH, FANOUT, dev)
        db.load(n_id, adjs)
        pool.append((db, labels[sd].contiguous()))
    return feats, pool


def make_step(dev, feats, group=None):
    """(model, optimiser, step): an eager SageTrainStep over pre-loaded batches, the clip inside the optimiser as in the CLI."""
    from graphpope_amd.optim import Adam
    from graphpope_amd.train import SageTrainStep
    model = make_model(dev)
    opt = Adam(model.parameters(), lr=LR, betas=BETAS, eps=EPS, max_grad_norm=MAX_NORM)
    return model, opt, SageTrainStep(model, opt, feats, BATCH, FANOUT, sampler=None, graph=False, seed=STEP_SEED, group=group)


def state_tensors(model, opt):
    """Weights, BatchNorm buffers and Adam moments, in a fixed order."""
    out = [p.detach() for p in model.parameters()] + [b.detach() for b in model.buffers()]
    for p in model.parameters():
        st = opt.state.get(p, {})
        out += [st[k] for k in ("exp_avg", "exp_avg_sq") if k in st]
    return out


def same_bits(a, b):
    """torch.equal on the bit patterns (a NaN equals itself, -0 differs from +0)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(a, b))


def flat_state(model, opt):
    return torch.cat([t.reshape(-1).to(torch.float32).contiguous().view(torch.int32) if t.dtype == torch.float32
                      else t.reshape(-1).to(torch.int32) for t in state_tensors(model, opt)])


# ------------------------------------------------------------------------------------------------ the CLI's data set
def write_pubmed_npz(directory, n=600, seed=5):
    """A PubMed-shaped .npz (500 features, 3 classes) of `n` nodes for GRAPHPOPE_DATA_DIR: half of the nodes train, a quarter validate."""
    import os
    from graphpope_amd import synth
    rng = np.random.RandomState(seed)
    ei = synth.powerlaw_graph(n, 4 * n, seed=seed, alpha=0.9, shift=0.8)       # symmetric, like PubMed
    split = rng.rand(n)
    np.savez(os.path.join(directory, "pubmed.npz"), x=rng.rand(n, 500).astype(np.float32), y=rng.randint(0, 3, n).astype(np.int64),
             edge_index=ei.astype(np.int64), train_mask=split < 0.5, val_mask=(split >= 0.5) & (split < 0.75), test_mask=split >= 0.75)
