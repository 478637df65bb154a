"""Data-parallel SAGE training: one process per GPU, the seeds split as Lightning's DistributedSampler splits them, the gradients
averaged over the ranks in ONE bucket (the reference: ``Trainer(gpus=args.n_gpus, accelerator='ddp', gradient_clip_val=0.5)``,
main.py:285-290).

torch's DistributedDataParallel is not used: the gradients here are fresh tensors handed out by hand-written autograd nodes, and the
optimiser is one launch over pointer tables.  What DDP does per step is instead spelled out between ``backward()`` and ``opt.step()``:

    pack      every live gradient * (1 / world) into one flat float32 buffer      one launch (csrc/grad_bucket.hip)
    reduce    dist.all_reduce(flat, SUM)                                          one collective
    install   p.grad = the parameter's view of the buffer                         no launch
    then      the squared norm of the AVERAGED gradient and the Adam step (optim.Adam(max_grad_norm=...)), as in a single process --
              Lightning clips after DDP's reduce, too.  Their pointer tables now see the same addresses every step.

A parameter without a gradient stays without one and is not in the bucket: the reference's default model has a third conv that never
runs (SURVEY §7 trap 7), which is why Lightning passes find_unused_parameters=True.  BatchNorm running statistics are not synchronised
during training (Lightning's default, no SyncBatchNorm); rank 0's are broadcast in front of every evaluation pass, which is what DDP's
broadcast_buffers=True amounts to for what evaluation sees.  Nothing here is captured into a HIP graph: see train.SageTrainStep.
"""
from __future__ import annotations

import ctypes

import torch
import torch.distributed as dist

from . import _lib
from ._lib import check, on_device


def world_size(group=None) -> int:
    """Ranks of `group` (None: the default group); 1 when no process group is initialised."""
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    return dist.get_world_size(group)


def bucket_layout(numel):
    """(offsets, total) of sage_grad_bucket_layout for a list of element counts: host logic, no GPU."""
    n = len(numel)
    nn = (ctypes.c_int64 * n)(*numel)
    off = (ctypes.c_int64 * n)()
    total = int(_lib.load().sage_grad_bucket_layout(n, nn, off))
    if total < 0:
        raise ValueError("sage_grad_bucket_layout: bad list of sizes")
    return list(off), total


class GradBucket:
    """The gradients of `params` in one flat float32 device tensor; see the module docstring.

    flat      float32 [total]: tensor t at offsets[t] (a multiple of 4 elements), up to three zeros of padding behind each
    views     one view of `flat` per live parameter, with the parameter's shape
    live      the parameters the bucket was built over: those that had a gradient at the last :meth:`pack`

    The bucket is rebuilt when the set of parameters with a gradient or a parameter's storage changes (the rule of optim.Adam._build);
    the addresses of the gradients themselves are refreshed at every :meth:`pack`, as Adam.step refreshes its own."""

    def __init__(self, params):
        self.params = list(params)
        self.flat = None
        self.views = []
        self.live = []
        self._tab = None

    def _build(self, live):
        for p in live:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError("graphpope_amd.parallel.GradBucket: float32 contiguous CUDA parameters only (no CPU fallback)")
        dev = live[0].device
        if any(p.device != dev for p in live):
            raise RuntimeError("graphpope_amd.parallel.GradBucket: all parameters on one device")
        n = len(live)
        numel = [p.numel() for p in live]
        offsets, total = bucket_layout(numel)
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.views = [self.flat[o:o + k].view(p.shape) for o, k, p in zip(offsets, numel, live)]
        self.live = live
        return {"ids": [id(p) for p in live], "pptr": [p.data_ptr() for p in live], "n": n, "nn": (ctypes.c_int64 * n)(*numel),
                "gg": (ctypes.c_void_p * n)(*([0] * n)), "gptr": [0] * n, "dev": dev, "total": total}

    def pack(self, scale: float = 1.0) -> None:
        """flat = every current ``p.grad`` * scale, in one library call (one launch per sage_grad_bucket_table() tensors)."""
        live = [p for p in self.params if p.grad is not None]
        if not live:
            self.flat, self.views, self.live, self._tab = None, [], [], None
            return
        tab = self._tab
        if (tab is None or tab["n"] != len(live) or any(a != id(b) for a, b in zip(tab["ids"], live))
                or any(a != b.data_ptr() for a, b in zip(tab["pptr"], live))):
            tab = self._tab = self._build(live)
        gptr, gg, keep = tab["gptr"], tab["gg"], []
        for i, p in enumerate(live):
            g = p.grad
            if not (g.is_cuda and g.dtype == torch.float32 and g.device == tab["dev"]):
                raise RuntimeError("graphpope_amd.parallel.GradBucket: float32 CUDA gradients only (no CPU fallback)")
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)                                   # alive until the launch is enqueued
            a = g.data_ptr()
            if a != gptr[i]:
                gptr[i] = a
                gg[i] = a
        with on_device(tab["dev"]):
            check(_lib.load().sage_grad_bucket_pack(tab["n"], gg, tab["nn"], float(scale), ctypes.c_void_p(self.flat.data_ptr()), tab["total"],
                                                    ctypes.c_void_p(torch.cuda.current_stream(tab["dev"]).cuda_stream)))

    def all_reduce(self, group=None) -> None:
        if self.flat is not None:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)

    def install(self) -> None:
        """``p.grad`` = the parameter's view of the bucket, for every live parameter."""
        for p, v in zip(self.live, self.views):
            p.grad = v

    def sync(self, group=None, force: bool = False) -> None:
        """Average the gradients over the ranks of `group`: pack(1 / world), all_reduce, install.  World 1 without `force`: nothing at
        all happens, the gradients stay the tensors backward() left."""
        world = world_size(group)
        if world == 1 and not force:
            return
        self.pack(1.0 / world)
        self.all_reduce(group)
        self.install()


def partition(node_idx: torch.Tensor, world: int, rank: int, shuffle: bool, seed: int, epoch: int) -> torch.Tensor:
    """This rank's share of `node_idx` for `epoch`, as ``DistributedSampler(range(len(node_idx)), num_replicas=world, rank=rank,
    shuffle=shuffle, seed=seed, drop_last=False)`` after ``set_epoch(epoch)`` picks it: the permutation of a CPU generator seeded
    ``seed + epoch`` (every rank draws the same one), padded by wrap-around to a multiple of `world`, then every world-th entry from
    `rank` on.  All ranks get equally many."""
    if not (world >= 1 and 0 <= rank < world):
        raise ValueError(f"partition: rank {rank} of world {world}")
    n = int(node_idx.numel())
    if n == 0:
        return node_idx
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(seed) + int(epoch))
        order = torch.randperm(n, generator=g)
    else:
        order = torch.arange(n)
    total = -(-n // world) * world
    if total > n:
        order = order.repeat(-(-total // n))[:total]
    return node_idx[order[rank:total:world].to(node_idx.device)]


def partition_eval(node_idx: torch.Tensor, world: int, rank: int) -> torch.Tensor:
    """``node_idx[rank::world]``: no padding, so every node is counted exactly once over the ranks.  (Lightning pads the evaluation
    splits like the training one and counts the duplicates; deliberately not done here)"""
    if not (world >= 1 and 0 <= rank < world):
        raise ValueError(f"partition_eval: rank {rank} of world {world}")
    return node_idx[rank::world]


def broadcast_parameters(model, group=None, src: int = 0) -> None:
    """Parameters and buffers of rank `src` to every rank, once at start-up."""
    with torch.no_grad():
        for t in list(model.parameters()) + list(model.buffers()):
            dist.broadcast(t, src=src, group=group)


def broadcast_buffers(model, group=None, src: int = 0) -> None:
    """The buffers (BatchNorm running_mean / running_var / num_batches_tracked) of rank `src` to every rank: in front of every
    evaluation pass, so that all ranks evaluate one model."""
    with torch.no_grad():
        for t in model.buffers():
            dist.broadcast(t, src=src, group=group)


def parameter_checksum(model) -> torch.Tensor:
    """Two int64 words over the bits of all parameters (their sum and a position-weighted sum): equal on ranks that hold equal weights."""
    with torch.no_grad():
        bits = torch.cat([p.detach().reshape(-1).view(torch.int32).to(torch.int64) for p in model.parameters()])
        weight = torch.arange(bits.numel(), device=bits.device, dtype=torch.int64) % 65521 + 1
        return torch.stack([bits.sum(), (bits * weight).sum()])


def assert_same_parameters(model, group=None) -> None:
    """Every rank compares :func:`parameter_checksum` with rank 0's (one 16-byte all-gather); RuntimeError on a difference."""
    mine = parameter_checksum(model)
    world = world_size(group)
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine, group=group)
    if not torch.equal(every[0], mine):
        raise RuntimeError(f"data-parallel training: the parameters of rank {dist.get_rank(group)} differ from rank 0's "
                           f"(checksum {mine.tolist()} against {every[0].tolist()})")
