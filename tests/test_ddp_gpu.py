"""Data-parallel SAGE training on the GPU: the bucket kernel alone through the C ABI, ranks that share one card over gloo (the pattern of
tests/test_distributed_gpu.py), the RCCL all-reduce on one rank, and the CLI with --n_gpus 2.

Nothing here runs on more than one GPU, and RCCL never with more than one rank: a one-GPU box cannot hold two RCCL ranks."""
import ctypes
import os
import signal
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ddp_cases as cases
from conftest import ROOT
from workspace import GuardedScratch, dev, lib  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEADLINE = 120.0


# ------------------------------------------------------------------------------------------------ the kernel alone
class PackCall:
    """Operands of one sage_grad_bucket_pack call between guard bands: every source in a buffer of its own (`shift` bytes off the
    16-byte grid), `flat` exactly the layout's length and pre-filled with NaN."""

    def __init__(self, dev, lib, sizes, seed, shift=0):
        self.lib, self.sizes = lib, list(sizes)
        self.grads = [cases.gradient_values(n, seed + 31 * t) for t, n in enumerate(self.sizes)]
        self.src = []
        for g in self.grads:
            s = GuardedScratch(dev, 4 * g.size + shift)
            if g.size:
                s.view[shift:].copy_(torch.from_numpy(g.view(np.uint8)))
            self.src.append(s)
        n = len(self.sizes)
        self.nn = (ctypes.c_int64 * n)(*self.sizes)
        self.gg = (ctypes.c_void_p * n)(*[s.ptr.value + shift if g.size else 0 for s, g in zip(self.src, self.grads)])
        self.total = lib.sage_grad_bucket_layout(n, self.nn, None)
        self.flat = GuardedScratch(dev, 4 * self.total)
        self.flat.view.copy_(torch.from_numpy(np.full(self.total, np.nan, dtype=np.float32).view(np.uint8)))
        self.before = [s.snapshot() for s in self.src]

    def run(self, scale, gg=None, flat=None, flat_len=None):
        return self.lib.sage_grad_bucket_pack(len(self.sizes), self.gg if gg is None else gg, self.nn, scale,
                                              self.flat.ptr if flat is None else flat, self.total if flat_len is None else flat_len,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def bits(self):
        return self.flat.view.cpu().numpy().view(np.uint32)

    def untouched(self):
        return self.flat.bands_intact() and all(s.unchanged_since(b) for s, b in zip(self.src, self.before))


@pytest.mark.parametrize("shift", [0, 4], ids=["aligned", "off_by_4_bytes"])
@pytest.mark.parametrize("scale", cases.SCALES, ids=["1", "half", "third", "eighth"])
def test_pack_is_the_scaled_gradients_bit_for_bit(dev, lib, scale, shift):
    """flat = np.float32(g) * np.float32(scale) bit for bit (one rounding, NaN, +-inf and +-0 included), the padding +0.0, the guard bands
    around flat and around every source untouched, at every size at which the kernel takes another path."""
    call = PackCall(dev, lib, cases.pack_sizes(lib.sage_grad_bucket_chunk()), seed=3, shift=shift)
    assert call.run(scale) == 0, lib.pope_last_error()
    got, want = call.bits(), cases.pack_expected(call.grads, scale)
    assert got.shape == want.shape and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert call.untouched()


def test_pack_takes_a_list_longer_than_one_descriptor_table(dev, lib):
    """More tensors than one launch's table holds, empty ones among them and a table boundary behind an empty one."""
    table, chunk = lib.sage_grad_bucket_table(), lib.sage_grad_bucket_chunk()
    sizes = [(0, 5, 1, 64, 3, 257, 0, 4)[t % 8] for t in range(2 * table + 7)]
    sizes[table] = 2 * chunk + 9                                           # several blocks in the second launch
    call = PackCall(dev, lib, sizes, seed=9)
    assert call.run(1.0 / 3.0) == 0, lib.pope_last_error()
    assert np.array_equal(call.bits(), cases.pack_expected(call.grads, 1.0 / 3.0)) and call.untouched()


def test_pack_refuses_bad_arguments_and_writes_nothing(dev, lib):
    from graphpope_amd import _lib
    call = PackCall(dev, lib, [5, 0, 257, 4], seed=1)
    nan_bits = np.full(call.total, np.nan, dtype=np.float32).view(np.uint32)
    hole = (ctypes.c_void_p * 4)(*call.gg)
    hole[2] = 0
    for kwargs in (dict(flat=ctypes.c_void_p(0)), dict(flat_len=call.total - 1), dict(gg=hole), dict(flat_len=0)):
        assert call.run(0.5, **kwargs) == _lib.ERR_INVALID, kwargs
        assert lib.pope_last_error().startswith(b"sage_grad_bucket_pack")
    torch.cuda.synchronize()
    assert np.array_equal(call.bits(), nan_bits) and call.untouched()      # on error nothing is launched
    assert call.run(0.5) == 0 and np.array_equal(call.bits(), cases.pack_expected(call.grads, 0.5))


# ------------------------------------------------------------------------------------------------ ranks that share the card
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(worker, world, backend, result_dir):
    """The ranks as fresh processes, joined against DEADLINE: a stuck collective ends as a failure, never as a hang."""
    ctx = mp.spawn(worker, args=(world, _free_port(), backend, str(result_dir)), nprocs=world, join=False)
    end = time.monotonic() + DEADLINE
    done = False
    try:
        while not done and time.monotonic() < end:
            done = ctx.join(timeout=1.0)
    finally:
        if not done:
            for p in ctx.processes:
                if p.is_alive():
                    p.terminate()
            for p in ctx.processes:
                p.join(10)
    assert done, f"the ranks did not finish within {DEADLINE:.0f} s"
    for r in range(world):
        assert open(os.path.join(result_dir, f"rank{r}")).read() == "ok"


def _enter(rank, world, port, backend):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group(backend, rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    return torch.device("cuda", 0), dist.group.WORLD


def _report(result_dir, rank, problems):
    open(os.path.join(result_dir, f"rank{rank}"), "w").write("ok" if not problems else "; ".join(problems))


def _spy(bucket, rec):
    """Look between the parts of GradBucket.sync: the raw gradients and the packed bucket of the first step, and the bucket behind the
    all-reduce."""
    from graphpope_amd import parallel
    pack, reduce_ = bucket.pack, bucket.all_reduce

    def spy_pack(scale=1.0):
        pack(scale)
        if "raw" not in rec:
            offsets, total = parallel.bucket_layout([p.numel() for p in bucket.live])
            raw = torch.zeros(total, dtype=torch.float32, device=bucket.flat.device)
            for o, p in zip(offsets, bucket.live):
                raw[o:o + p.numel()] = p.grad.reshape(-1)
            rec["raw"], rec["scale"] = raw, scale

    def spy_reduce(group=None):
        first = "local" not in rec
        if first:
            rec["local"] = bucket.flat.clone()
        reduce_(group)
        if first:
            rec["reduced"] = bucket.flat.clone()

    bucket.pack, bucket.all_reduce = spy_pack, spy_reduce


def _gather(t, world, group):
    every = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(every, t.contiguous(), group=group)
    return every


def _two_rank_worker(rank, world, port, backend, result_dir):
    import sage_model_cases as model_cases
    from graphpope_amd import sage
    from graphpope_amd.sage import EvalMetrics
    dev, group = _enter(rank, world, port, backend)
    bad = []
    try:
        with sage.deterministic(True):
            feats, pool = cases.make_data(dev, 6)
            # ---- check 1: the same batch on both ranks = the single-process step, bit for bit (fl(g/2 + g/2) = g)
            model, opt, step = cases.make_step(dev, feats, group)
            plain_model, plain_opt, plain = cases.make_step(dev, feats)
            assert step.bucket is not None and plain.bucket is None
            for i in range(3):
                for s in (step, plain):
                    s.load_batch(*pool[i])
                    s.run()
            a, b = cases.state_tensors(model, opt), cases.state_tensors(plain_model, plain_opt)
            if len(a) != len(b) or not all(cases.same_bits(x, y) for x, y in zip(a, b)):
                bad.append("check 1: the two-rank step on one batch differs from the single-process step")
            if not cases.same_bits(step.loss, plain.loss):
                bad.append("check 1: the loss differs")
            # ---- check 2: different batches
            model, opt, step = cases.make_step(dev, feats, group)
            rec = {}
            _spy(step.bucket, rec)
            start = [p.detach().clone() for p in model.parameters()]
            step.load_batch(*pool[rank])
            step.run()
            after1 = [p.detach().clone() for p in model.parameters()]
            coef = float(opt.clip_coef)
            locals_ = _gather(rec["local"], world, group)
            if rec["scale"] != 0.5:
                bad.append(f"check 2: packed with scale {rec['scale']}")
            if not cases.same_bits(rec["reduced"], locals_[0] + locals_[1]):
                bad.append("check 2: the bucket behind the all-reduce is not fl(b0 + b1)")
            live_ids = {id(p) for p in step.bucket.live}
            for k, (p, p0, p1) in enumerate(zip(model.parameters(), start, after1)):
                if id(p) not in live_ids:
                    continue
                g = step.bucket.views[[id(q) for q in step.bucket.live].index(id(p))]
                if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                    bad.append(f"check 2: parameter {k}'s gradient is not its view of the bucket")
                zero = np.zeros(p.numel())
                want, bound = model_cases.adam_reference(p0.cpu().numpy().ravel(), g.cpu().numpy().ravel(), zero, zero, coef, cases.LR,
                                                         *cases.BETAS, cases.EPS, 1)
                err = np.abs(p1.cpu().numpy().ravel().astype(np.float64) - want)
                if not (err <= bound).all():
                    bad.append(f"check 2: parameter {k} moved {float((err / bound).max()):.3g} bounds from the float64 Adam step")
            for i in (1, 2):
                step.load_batch(*pool[2 * i + rank])
                step.run()
            every = _gather(cases.flat_state(model, opt)[: sum(p.numel() for p in model.parameters())], world, group)
            if not torch.equal(every[0], every[1]):
                bad.append("check 2: the weights differ between the ranks after three steps")
            moments = torch.cat([opt.state[p][k].reshape(-1).view(torch.int32) for p in step.bucket.live for k in ("exp_avg", "exp_avg_sq")])
            every = _gather(moments, world, group)
            if not torch.equal(every[0], every[1]):
                bad.append("check 2: the Adam moments differ between the ranks after three steps")
            unused = list(model.convs[2].parameters())
            fresh = list(cases.make_model(dev).convs[2].parameters())
            if not unused or any(p.grad is not None for p in unused) or any(id(p) in live_ids for p in unused):
                bad.append("check 2: the conv that never runs has a gradient")
            if not all(cases.same_bits(p.detach(), q.detach()) for p, q in zip(unused, fresh)):
                bad.append("check 2: the conv that never runs changed")
            # ---- check 4: metrics
            gen = torch.Generator().manual_seed(77)
            parts = [(torch.randn(n, cases.CLASSES, generator=gen).to(dev), torch.randint(0, cases.CLASSES, (n,), generator=gen).to(dev))
                     for n in (37, 52)]
            single, each = EvalMetrics(dev), [EvalMetrics(dev), EvalMetrics(dev)]
            for r, (logits, y) in enumerate(parts):
                single.update(logits, y)
                each[r].update(logits, y)
            sums = [float(m.acc.cpu().numpy()[:1].view(np.float64)[0]) for m in each]
            mine = each[rank]
            mine.all_reduce(group)
            words, want = mine.acc.cpu().numpy(), single.acc.cpu().numpy()
            if int(words[1]) != int(want[1]) or int(words[2]) != int(want[2]) or int(words[2]) != 89:
                bad.append(f"check 4: correct / rows {words[1:].tolist()} against {want[1:].tolist()}")
            loss_sum = float(words[:1].view(np.float64)[0])
            if not abs(loss_sum - (sums[0] + sums[1])) <= 4 * 2.0 ** -53 * (abs(sums[0]) + abs(sums[1])):
                bad.append(f"check 4: loss sum {loss_sum!r} against {sums[0]!r} + {sums[1]!r}")
        _report(result_dir, rank, bad)
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_card(tmp_path):
    """Checks 1, 2 and 4 of the issue in one spawn of two gloo ranks on cuda:0; see _two_rank_worker."""
    _spawn(_two_rank_worker, 2, "gloo", tmp_path)


def _three_rank_worker(rank, world, port, backend, result_dir):
    from graphpope_amd import sage
    dev, group = _enter(rank, world, port, backend)
    bad = []
    try:
        with sage.deterministic(True):
            feats, pool = cases.make_data(dev, 3)
            model, opt, step = cases.make_step(dev, feats, group)
            rec = {}
            _spy(step.bucket, rec)
            step.load_batch(*pool[rank])
            step.run()
            raws = [r.cpu().numpy().astype(np.float64) for r in _gather(rec["raw"], world, group)]
            mean = sum(raws) / world
            bound = (world + 1) * 2.0 ** -24 * sum(np.abs(r) for r in raws) / world
            err = np.abs(rec["reduced"].cpu().numpy().astype(np.float64) - mean)
            if not (err <= bound).all():
                at = int(np.argmax(err - bound))
                bad.append(f"check 3: element {at} is {err[at]:.3g} from the float64 mean, bound {bound[at]:.3g}")
            if not (np.abs(mean) > 0).any() or rec["scale"] != 1.0 / 3.0:
                bad.append("check 3: nothing was averaged")
        _report(result_dir, rank, bad)
    finally:
        dist.destroy_process_group()


def test_three_ranks_average_within_the_rounding_bound(tmp_path):
    """Check 3: the bucket behind the all-reduce within (W + 1) * 2^-24 * sum_r |g_r| / W of the float64 mean of the ranks' float32
    gradients, element by element (W roundings of the pre-scale, W - 1 additions in unknown order, one unit for second-order terms)."""
    _spawn(_three_rank_worker, 3, "gloo", tmp_path)


def _rccl_worker(rank, world, port, backend, result_dir):
    from graphpope_amd import sage
    from graphpope_amd.parallel import GradBucket
    dev, group = _enter(rank, world, port, backend)
    bad = []
    try:
        with sage.deterministic(True):
            feats, pool = cases.make_data(dev, 2)
            model, opt, step = cases.make_step(dev, feats, group)
            plain_model, plain_opt, plain = cases.make_step(dev, feats)
            if step.bucket is not None:
                bad.append("check 5: a group of one rank built a bucket")
            probe = GradBucket(model.parameters())
            probe.sync(group)                                               # world 1, no force: nothing at all
            if probe.flat is not None:
                bad.append("check 5: sync without force did something")
            step.group, step.bucket = group, GradBucket(step.params)        # the step's own hook, forced through RCCL
            sync, seen = step.bucket.sync, {}

            def forced(g=None):
                seen["before"] = [None if p.grad is None else p.grad.detach().clone() for p in step.params]
                sync(g, force=True)
                seen["after"] = [None if p.grad is None else p.grad.detach().clone() for p in step.params]

            step.bucket.sync = forced
            for i in range(2):
                for s in (step, plain):
                    s.load_batch(*pool[i])
                    s.run()
            same = all((x is None and y is None) or (x is not None and y is not None and cases.same_bits(x, y))
                       for x, y in zip(seen["before"], seen["after"]))
            if not same or all(x is None for x in seen["after"]):
                bad.append("check 5: sync(force=True) on one rank changed the gradients")
            a, b = cases.state_tensors(model, opt), cases.state_tensors(plain_model, plain_opt)
            if len(a) != len(b) or not all(cases.same_bits(x, y) for x, y in zip(a, b)):
                bad.append("check 5: the step behind the RCCL all-reduce differs from the plain step")
        _report(result_dir, rank, bad)
    finally:
        dist.destroy_process_group()


def test_rccl_all_reduce_runs_on_one_rank(tmp_path):
    """Check 5: world 1 on the nccl backend -- GradBucket.sync(force=True) runs the RCCL all-reduce once on the GPU, leaves the gradients
    bit-identical, and the step behind it equals the plain step bit for bit."""
    _spawn(_rccl_worker, 1, "nccl", tmp_path)


# ------------------------------------------------------------------------------------------------ the CLI
def _cli(env, limit=240.0):
    cmd = [sys.executable, "-m", "graphpope_amd.main", "--n_gpus", "2", "--dataset", "pubmed", "--epochs", "2", "--batch_size", "64",
           "--num_anchor_nodes", "8", "--sampling_method", "stochastic"]
    proc = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)                                 # the launcher and the ranks with it
        proc.communicate()
        pytest.fail(f"python -m graphpope_amd.main --n_gpus 2 did not finish within {limit:.0f} s")
    assert proc.returncode == 0, err[-4000:]
    # the program's own lines; the gloo library writes "[Gloo] Rank ..." notes of its own to the same stream, from both ranks at once
    return [line for line in out.splitlines() if line.startswith(("Namespace(", "epoch ", "test_acc "))]


def test_cli_trains_on_two_ranks(tmp_path):
    """python -m graphpope_amd.main --n_gpus 2 without a launcher: the parent starts two gloo ranks on the one card; exit 0, each epoch
    line and the test_acc line exactly once (only rank 0 prints), and a second run prints the same lines to the character.  Every rank
    compares its parameters with rank 0's before it returns."""
    cases.write_pubmed_npz(str(tmp_path))
    env = dict(os.environ, GRAPHPOPE_DDP_BACKEND="gloo", GRAPHPOPE_DETERMINISTIC="1", GRAPHPOPE_DATA_DIR=str(tmp_path),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    first = _cli(env)
    for head in ("epoch 0:", "epoch 1:", "test_acc "):
        assert sum(line.startswith(head) for line in first) == 1, (head, first)
    assert sum(line.startswith("Namespace(") for line in first) == 1
    losses = [float(line.split("train_loss ")[1].split()[0]) for line in first if line.startswith("epoch ")]
    assert len(first) == 4 and all(np.isfinite(losses))
    assert _cli(env) == first
