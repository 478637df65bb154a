"""One GraphSAGE training step with no host in the loop: sampled, run and optimised entirely by kernels that read their
sizes on the device, captured once into a HIP graph and replayed.

What the reference does per step (/root/reference/main.py): a DataLoader worker samples the batch
(NeighborSampler(sizes=[25, 10]), main.py:100-116) and gathers ``data.x[n_id]`` (convert_batch, main.py:118-123);
Lightning moves it to the GPU, calls ``training_step`` (main.py:213-222: forward + ``F.cross_entropy``), backward,
clips the gradient norm to 0.5 (main.py:286) and steps Adam (main.py:244).  Here the same step is

    sample (device-extent sampler, no read-back)  ->  SAGE forward on IndexedFeatures  ->  cross-entropy
    ->  backward  ->  squared gradient norm (one launch)  ->  one-launch Adam, clip coefficient formed in its prologue
    ->  advance the device-side seeds / step count

with the optimiser built as ``Adam(..., max_grad_norm=0.5)``.  (``clip=`` of :class:`SageTrainStep` is the older form, torch's
``clip_grad_norm_`` between backward and a plain Adam: a chain of small launches that rewrites every gradient.)  The step is
enqueued once through the ordinary autograd path while a HIP graph is being captured, then replayed: a step costs one
small launch that loads the seeds and labels plus one graph launch.  Batches come either from the device sampler inside
the graph (`sampler` given) or from a pool of pre-sampled batches loaded into the graph's fixed buffers
(:meth:`load_batch`).  The data-dependent sizes of a batch never reach the host (include/graphpope_hip.h, "Device
extents"), so nothing in the step synchronises.

Reproducibility.  Every kernel of the step but one is a pure function of its inputs; the exception is the float-atomic scatter of the
hidden layer's input gradient (csrc/sage.hip: k_scatter_mean), whose additions land in arrival order, so two runs of a step may differ
in their last bits.  ``sage.set_deterministic(True)`` replaces it by a per-source sum in a fixed order (and makes the evaluation
metrics add once per launch): eager and replayed steps then give the same bits, run after run.  Both step classes below record the mode
they were built under as ``.deterministic``; the mode is read when the launches are enqueued, so a captured graph keeps the mode it was
captured under whatever the switch says later -- build the step inside the mode it is to run in.  ``prefetch=True`` (a second stream
samples ahead) is not covered by the mode.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import check, on_device
from .parallel import GradBucket, world_size
from .sage import EvalMetrics, IndexedFeatures, cross_entropy, is_deterministic
from .sampler import DeviceBatch

_SEED_STRIDE = 0x9E3779B97F4A7C15 % (1 << 63)        # odd: the seed words walk through all 2^64 values


class StepState:
    """Four device words a replayed step reads and one launch advances: dropout seed, sampling seed, Adam step count, and
    the position in the epoch's node order (epoch mode: the next batch's seeds start there)."""

    def __init__(self, device, seed: int = 0, adam_step: int = 0):
        self.words = torch.tensor([seed, seed ^ 0x5DEECE66D, adam_step + 1, 0], dtype=torch.int64, device=device)
        self._inc = (ctypes.c_int64 * 4)(_SEED_STRIDE, _SEED_STRIDE | 2, 1, 0)
        self._inc_keep_sample = (ctypes.c_int64 * 4)(_SEED_STRIDE, 0, 1, 0)
        self._inc_only_sample = (ctypes.c_int64 * 4)(0, _SEED_STRIDE | 2, 0, 0)

    dropout_seed = property(lambda self: self.words[0:1])
    sample_seed = property(lambda self: self.words[1:2])
    adam_step = property(lambda self: self.words[2:3])
    cursor = property(lambda self: self.words[3:4])

    def advance(self, sample_seed: bool = True, cursor_by: int = 0) -> None:
        lib = _lib.load()
        inc = self._inc if sample_seed else self._inc_keep_sample
        if cursor_by:
            inc = (ctypes.c_int64 * 4)(inc[0], inc[1], inc[2], cursor_by)
        with on_device(self.words.device):
            check(lib.sage_advance_counters(ctypes.c_void_p(self.words.data_ptr()), inc, 4,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def advance_sample_seed(self) -> None:
        """Only the sampling seed (a batch sampled ahead on a side stream advances it there, in sampling order)."""
        lib = _lib.load()
        with on_device(self.words.device):
            check(lib.sage_advance_counters(ctypes.c_void_p(self.words.data_ptr()), self._inc_only_sample, 4,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def copy_segments(dst, src) -> None:
    """dst[i][:] = src[i] for lists of contiguous device tensors (src[i] may be shorter than dst[i]) in ONE launch."""
    lib = _lib.load()
    n = len(dst)
    assert n == len(src)
    arr = ctypes.c_void_p * n
    nbytes = []
    for d, s in zip(dst, src):
        assert d.is_cuda and s.is_cuda and d.is_contiguous() and s.is_contiguous() and d.dtype == s.dtype
        assert s.numel() <= d.numel()
        nbytes.append(s.numel() * s.element_size())
    with on_device(dst[0].device):
        check(lib.sage_copy_segments(n, arr(*[d.data_ptr() for d in dst]), arr(*[s.data_ptr() for s in src]),
                                     (ctypes.c_int64 * n)(*nbytes), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


class SageTrainStep:
    """``step(seeds, y)`` = one optimiser step of `model` on the batch around `seeds`; see the module docstring.

    model      graphpope_amd.sage.SAGE (training mode is set here)
    opt        graphpope_amd.optim.Adam over model.parameters()
    feats      float32 [N, C] on the device: features (+) POPE, resident in HBM
    sampler    graphpope_amd.sampler.NeighborSampler, or None: batches are then loaded with :meth:`load_batch`
    clip       max gradient norm (Lightning's gradient_clip_val) applied with torch.nn.utils.clip_grad_norm_, or None.  The clip of
               the optimiser itself (Adam(max_grad_norm=...)) is the cheaper way; giving both raises ValueError (it would clip twice)
    graph      False: the same step, enqueued eagerly every time (A/B and debugging)
    group      a torch.distributed process group of more than one rank: data-parallel training (graphpope_amd.parallel).  The body then
               averages the gradients over the ranks (GradBucket.sync: pack, all-reduce, install) between backward() and the clip /
               opt.step(), so the norm is the averaged gradient's, as Lightning clips behind DDP's reduce.  Such a step is ALWAYS
               enqueued eagerly, whatever `graph` says -- a decision, not an omission: a gloo collective cannot be captured, a captured
               RCCL collective has never run here, and the eager sampled step is within 3 % of the replayed one (README).  ``loss`` is
               the loss of this rank's batch.  None, or a group of one rank: the single-process step, unchanged

    ``deterministic``: sage.is_deterministic() at construction.  A captured graph keeps the mode it was captured under.
    """

    def __init__(self, model, opt, feats: torch.Tensor, batch_size: int, sizes=(25, 10), sampler=None, clip: float | None = None,
                 graph: bool = True, seed: int = 0, prefetch: bool = False, group=None):
        if clip is not None and getattr(opt, "max_grad_norm", None) is not None:
            raise ValueError("SageTrainStep: clip and the optimiser's max_grad_norm are both set; the gradients would be clipped twice")
        dev = feats.device
        self.model, self.opt, self.feats, self.sampler, self.clip = model, opt, feats, sampler, clip
        self.deterministic = is_deterministic()
        self.batch = DeviceBatch(batch_size, sizes if sampler is None else sampler.sizes, dev)
        self.seeds = torch.zeros(batch_size, dtype=torch.int64, device=dev)
        self.y = torch.zeros(batch_size, dtype=torch.int64, device=dev)
        self.state = StepState(dev, seed)
        self.params = [p for p in model.parameters()]
        self.loss = None
        self.logits = None
        self._one = torch.ones((), device=dev)
        self._side = torch.cuda.Stream(device=dev)                   # warm-up calls and the capture run here
        self._graph = None
        self._use_graph = graph
        self._lr = None
        self._calls = 0
        self.group, self.bucket = None, None
        if group is not None and world_size(group) > 1:              # data-parallel: eager, with the gradient bucket in the body
            self.group, self.bucket = group, GradBucket(self.params)
            self._use_graph = False
        # epoch mode (set_epoch / step_epoch): the step draws its own seeds and labels from device-resident tables
        self._epoch_mode = False
        self._order = self._labels = None
        self._epoch_len = self._epoch_pos = 0
        # prefetch (sampler given, graph=False): the NEXT batch is sampled on a side stream while this step computes -- the
        # reference's DataLoader workers do the same on the host (main.py:100-104, persistent_workers).  Two batch buffers.
        self._prefetch = bool(prefetch and sampler is not None and not graph)
        if self._prefetch:
            self._batches = [self.batch, DeviceBatch(batch_size, sampler.sizes, dev)]
            self._ys = [self.y, torch.zeros_like(self.y)]
            self._sample_stream = torch.cuda.Stream(device=dev)
            self._ready = None          # (event, buffer index) of the batch sampled ahead
            self._free = [None, None]   # per buffer: event behind the last step that read it
        model.dropout_seed_dev = self.state.dropout_seed
        opt.use_device_step(self.state.adam_step)

    # ---- the step body: ordinary autograd code, capturable ----
    def _body(self, sample: bool = True):
        if self.sampler is not None and sample:
            if self._epoch_mode:
                self.sampler.sample_epoch_device(self._order, self.state.cursor, self._labels, self.y, seed=0, out=self.batch,
                                                 seed_dev=self.state.sample_seed)
            else:
                self.sampler.sample_device(self.seeds, seed=0, out=self.batch, seed_dev=self.state.sample_seed)
        x = IndexedFeatures(self.feats, self.batch.n_id)             # main.py:118-123 without the copy
        for p in self.params:
            p.grad = None
        logits = self.model(x, self.batch.adjs)
        loss = cross_entropy(logits, self.y, unit_upstream=True, loss_in=self.opt)   # main.py:216; the backward pass below is seeded with 1, the scalar is finished by opt.step()'s launch
        loss.backward(gradient=self._one)
        # detached views of the results: nothing outside this call keeps the autograd graph (and its AccumulateGrad nodes,
        # which remember the stream they were created on) alive into the next call or into the capture
        self.logits, self.loss = logits.detach(), loss.detach()
        del logits, loss
        if self.bucket is not None:
            self.bucket.sync(self.group)                             # p.grad = the mean over the ranks, in the bucket
        if self.clip is not None:
            torch.nn.utils.clip_grad_norm_(self.params, self.clip)   # main.py:286 gradient_clip_val
        self.opt.step()
        self.state.advance(sample_seed=sample, cursor_by=self.batch.n_seeds if self._epoch_mode else 0)

    def _capture(self):
        self.loss = self.logits = None
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self._side):
            self._body()
        self._graph = g
        self._lr = [grp["lr"] for grp in self.opt.param_groups]
        for tab in self.opt._tables.values():                        # the captured opt.step() counted a step that did not run
            tab["step"] -= 1
            for st in tab["states"]:
                st["step"] = tab["step"]

    def _run(self):
        self.model.train(True)
        if not self._use_graph:
            self._body()
            return
        if self._graph is not None and self._lr != [grp["lr"] for grp in self.opt.param_groups]:
            self._graph = None                                       # the scheduler changed lr: it is a launch argument
        if self._graph is None:
            if self._calls < 2:                                      # first calls eager: lazy initialisations (LDS opt-ins,
                self._calls += 1                                     # side streams, Adam state) happen outside the capture --
                cur = torch.cuda.current_stream()                    # on the stream the capture will use, as torch asks
                self._side.wait_stream(cur)
                with torch.cuda.stream(self._side), torch.autograd.set_multithreading_enabled(False):
                    self._body()
                cur.wait_stream(self._side)
                return
            with torch.autograd.set_multithreading_enabled(False):
                self._capture()
        self._graph.replay()
        # the host-side step counters of the optimiser follow the replays
        for tab in self.opt._tables.values():
            tab["step"] += 1
            for st in tab["states"]:
                st["step"] = tab["step"]

    def _sample_ahead(self, seeds, y, idx):
        """Enqueue the sampling of (seeds, y) into buffer idx on the side stream; returns the event behind it."""
        cur = torch.cuda.current_stream()
        side = self._sample_stream
        side.wait_stream(cur)                                        # seeds / y were produced on the caller's stream
        if self._free[idx] is not None:
            side.wait_event(self._free[idx])                         # the step that last read this buffer is done
        with torch.cuda.stream(side):
            copy_segments([self._ys[idx]], [y])
            self.sampler.sample_device(seeds.contiguous(), seed=0, out=self._batches[idx], seed_dev=self.state.sample_seed)
            self.state.advance_sample_seed()
            ev = torch.cuda.Event()
            ev.record(side)
        return ev

    def step(self, seeds: torch.Tensor, y: torch.Tensor, next_seeds: torch.Tensor | None = None, next_y: torch.Tensor | None = None):
        """Sample around `seeds` (device int64 [batch_size]) inside the step, labels `y` (device int64 [batch_size]).
        With prefetch=True, `next_seeds` / `next_y` (the batch of the NEXT call) are sampled on a side stream meanwhile."""
        assert self.sampler is not None, "no sampler: use load_batch() + run()"
        if self._epoch_mode:                                         # back to caller-provided seeds: another graph
            self._epoch_mode, self._graph, self._calls = False, None, 0
        if not self._prefetch:
            copy_segments([self.seeds, self.y], [seeds, y])
            self._run()
            return self.loss
        cur = torch.cuda.current_stream()
        if self._ready is None:                                      # first call: nothing was sampled ahead
            self._ready = (self._sample_ahead(seeds, y, 0), 0)
        ev, idx = self._ready
        cur.wait_event(ev)
        self.batch, self.y = self._batches[idx], self._ys[idx]
        self._ready = None
        if next_seeds is not None:
            self._ready = (self._sample_ahead(next_seeds, next_y, idx ^ 1), idx ^ 1)
        self.model.train(True)
        self._body(sample=False)
        done = torch.cuda.Event()
        done.record(cur)
        self._free[idx] = done
        return self.loss

    # ---- epoch mode: the loader's part of an epoch on the device too (main.py:100-123) ----
    def set_epoch(self, order: torch.Tensor, labels: torch.Tensor) -> None:
        """Start an epoch over `order` (device int64: the training nodes in this epoch's -- shuffled -- order; the reference's
        NeighborSampler(node_idx, batch_size, shuffle=True)) with `labels` (device int64 [N]: data.y).  :meth:`step_epoch` then
        trains on consecutive slices of batch_size nodes without any per-step input: the position lives in a device word the
        replayed step advances, the labels of a batch are gathered by the sampler's first kernel."""
        assert self.sampler is not None and order.is_cuda and order.dtype == torch.int64 and labels.is_cuda and labels.dtype == torch.int64
        if self._order is None or self._order.numel() < order.numel() or self._labels.numel() != labels.numel():
            self._order = torch.empty(max(order.numel(), 1), dtype=torch.int64, device=order.device)
            self._labels = torch.empty_like(labels)
            self._graph = None                                       # other buffers: the capture has to be redone
        if not self._epoch_mode:
            self._graph = None
            self._calls = 0
        self._epoch_mode = True
        copy_segments([self._order, self._labels, self.state.words[3:4]], [order.contiguous(), labels.contiguous(),
                                                                          torch.zeros(1, dtype=torch.int64, device=order.device)])
        self._epoch_len, self._epoch_pos = order.numel(), 0

    def batches_left(self) -> int:
        """Full batches the current epoch still holds (a shorter tail is the caller's, as in main.py's eager tail batch)."""
        return (self._epoch_len - self._epoch_pos) // self.batch.n_seeds

    def step_epoch(self):
        """One step on the next batch_size nodes of the epoch's order; the batch's node ids are self.batch.n_id[:batch_size]."""
        assert self._epoch_mode and self.batches_left() > 0, "set_epoch() first; the epoch's full batches are used up"
        self._run()
        self._epoch_pos += self.batch.n_seeds
        return self.loss

    def load_batch(self, pooled: DeviceBatch, y: torch.Tensor) -> None:
        """A batch of a pre-sampled pool (DeviceBatch.load) into the step's fixed buffers: one launch."""
        copy_segments(self.batch.segments() + [self.y], pooled.segments(valid_only=True) + [y])

    def run(self):
        """The step on whatever :meth:`load_batch` put into the buffers."""
        assert self.sampler is None
        self._run()
        return self.loss


class SageEvalStep:
    """The forward-only step of a validation / test pass (main.py:224-241: ``validation_step`` / ``test_step`` over
    ``NeighborSampler(node_idx, shuffle=False)``), with no host in the loop: captured once, replayed once per batch.

        ev = SageEvalStep(model, feats, batch_size, sampler)
        mean_loss, acc = ev.run_pass(order, labels, sample_seed)

    The body, under ``torch.no_grad()`` with the model in eval mode (BatchNorm normalises with its running statistics, no dropout):

        sample the next batch_size nodes of `order` (device-extent sampler; its first kernel gathers their labels)
        ->  SAGE forward on IndexedFeatures  ->  sage_eval_metrics  ->  advance the sampling seed by 1 and the cursor by batch_size

    Batch b of a pass is the batch ``sampler.sample(order[b * batch_size : (b + 1) * batch_size], sample_seed + b)`` draws.  The step owns
    every device word it writes -- `words` = {sampling seed, cursor, loss sum, correct, rows}, its DeviceBatch with the sampler scratch
    inside, its label buffer -- and shares none with a SageTrainStep; weights and running statistics are read where the model keeps
    them, so a replay sees what training has written since the capture, and nothing about the optimiser is baked in.
    graph=False: the same body, enqueued eagerly every time (A/B and debugging).  max_nodes: the longest `order` any pass will bring
    (one step serves the validation and the test split); a longer one still works, at the price of a new capture.
    ``deterministic``: sage.is_deterministic() at construction (the loss sum of a pass is then reproducible to the bit); a captured
    graph keeps the mode it was captured under."""

    def __init__(self, model, feats: torch.Tensor, batch_size: int, sampler, graph: bool = True, max_nodes: int = 0):
        dev = feats.device
        self.model, self.feats, self.sampler = model, feats, sampler
        self.deterministic = is_deterministic()
        self._max_nodes = int(max_nodes)                             # the longest `order` to expect: a longer one re-captures
        self.batch = DeviceBatch(batch_size, sampler.sizes, dev)
        self.y = torch.zeros(batch_size, dtype=torch.int64, device=dev)
        self.words = torch.zeros(5, dtype=torch.int64, device=dev)
        self.metrics = EvalMetrics(dev, acc=self.words[2:5])
        self.logits = None                                           # the last full batch's logits [batch_size, C]
        self.tail_logits = None                                      # the last pass's tail batch, if it had one
        self.rows = 0
        self._inc = (ctypes.c_int64 * 2)(1, int(batch_size))
        self._order = self._labels = None
        self._len = self._pos = 0
        self._sample_seed = 0
        self._side = torch.cuda.Stream(device=dev)                   # warm-up calls and the capture run here
        self._graph = None
        self._use_graph = graph
        self._calls = 0

    sample_seed = property(lambda self: self.words[0:1])
    cursor = property(lambda self: self.words[1:2])

    def _body(self):
        self.sampler.sample_epoch_device(self._order, self.cursor, self._labels, self.y, seed=0, out=self.batch, seed_dev=self.sample_seed)
        self.logits = self.model(IndexedFeatures(self.feats, self.batch.n_id), self.batch.adjs)
        self.metrics.update(self.logits, self.y)
        with on_device(self.words.device):
            check(_lib.load().sage_advance_counters(ctypes.c_void_p(self.words.data_ptr()), self._inc, 2,
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def _run(self):
        if not self._use_graph:
            self._body()
            return
        if self._graph is None:
            if self._calls < 2:                                      # first calls eager, on the stream the capture will use
                self._calls += 1                                     # (lazy initialisations happen outside the capture)
                cur = torch.cuda.current_stream()
                self._side.wait_stream(cur)
                with torch.cuda.stream(self._side):
                    self._body()
                cur.wait_stream(self._side)
                return
            self.logits = None
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self._side):
                self._body()
            self._graph = g
        self._graph.replay()

    def begin_pass(self, order: torch.Tensor, labels: torch.Tensor, sample_seed: int) -> None:
        """Load `order` (device int64: the split's nodes), `labels` (device int64 [N]: data.y), cursor = 0, the sampling seed and
        zeroed metrics: one launch.  :meth:`step` then evaluates consecutive slices of batch_size nodes."""
        assert order.is_cuda and order.dtype == torch.int64 and labels.is_cuda and labels.dtype == torch.int64 and order.numel() > 0
        if self._order is None or self._order.numel() < order.numel() or self._labels.numel() != labels.numel():
            self._order = torch.empty(max(order.numel(), self._max_nodes), dtype=torch.int64, device=order.device)
            self._labels = torch.empty_like(labels)
            self._graph = None                                       # other buffers: the capture has to be redone
        init = torch.tensor([int(sample_seed), 0, 0, 0, 0], dtype=torch.int64).to(order.device)
        copy_segments([self._order, self._labels, self.words], [order.contiguous(), labels.contiguous(), init])
        self._len, self._pos, self._sample_seed = order.numel(), 0, int(sample_seed)

    def batches_left(self) -> int:
        """Full batches the pass still holds (a shorter tail is evaluated with host-known sizes, :meth:`run_pass`)."""
        return (self._len - self._pos) // self.batch.n_seeds

    def step(self) -> torch.Tensor:
        """Evaluate the next batch_size nodes of the pass; returns their logits (also self.logits; the batch's nodes are
        self.batch.n_id, its labels self.y).  The caller keeps the model in eval mode: :meth:`run_pass` does."""
        assert self._order is not None and self.batches_left() > 0, "begin_pass() first; the pass's full batches are used up"
        assert not self.model.training, "SageEvalStep.step: model.eval() first (run_pass does it)"
        with torch.no_grad():
            self._run()
        self._pos += self.batch.n_seeds
        return self.logits

    def run_pass(self, order: torch.Tensor, labels: torch.Tensor, sample_seed: int):
        """(mean loss, accuracy) over `order`: one replay per full batch, the shorter tail batch -- if any -- through the host-sized
        sampler onto the same device words, one 24-byte read-back.  ``self.rows`` = rows counted.  The model's training flag is
        restored; parameters, gradients, running statistics, optimiser state and the dropout seed are not written."""
        was_training = self.model.training
        self.model.train(False)
        try:
            self.begin_pass(order, labels, sample_seed)
            while self.batches_left():
                self.step()
            if self._pos < self._len:
                seeds = order[self._pos:].contiguous()
                n_id, adjs = self.sampler.sample(seeds, seed=self._sample_seed + self._pos // self.batch.n_seeds)
                with torch.no_grad():
                    self.tail_logits = self.model(IndexedFeatures(self.feats, n_id), adjs)
                self.metrics.update(self.tail_logits, labels.index_select(0, seeds))
                self._pos = self._len
        finally:
            self.model.train(was_training)
        loss, acc, self.rows = self.metrics.read()
        return loss, acc
