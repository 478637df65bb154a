"""Command-line front end with the reference's flag surface (/root/reference/main.py:31-52), verbatim.

    python -m graphpope_amd.main --dataset flickr --embedding_space geodesic --sampling_method stochastic \
        --num_anchor_nodes 256 --num_layers 3 --epochs 5

Same 15 flags, names, types and defaults -- including ``--wandb_logging`` being ``type=bool`` (any
non-empty string is True, main.py:49) and ``--dropout`` being parsed but never handed to the model
(main.py:272).  ``--embedding_space baseline`` skips GraphPOPE (main.py:94).

What differs, because PyG / Lightning / the datasets are not available offline: the graph comes from
``<--data_dir or ./data>/<dataset>.npz`` (arrays ``x, y, edge_index, train_mask, val_mask, test_mask``) if present
and otherwise from a synthetic graph of the dataset's shape; the Lightning ``Trainer`` is a plain loop with the
same optimiser, scheduler, clipping and early stopping (main.py:243-255, 279-290).  Flags are parsed in ``main()``
rather than at import.  ``GRAPHPOPE_DETERMINISTIC=1`` (an environment variable, like ``GRAPHPOPE_TRAIN_STEP``: the flag
surface stays the reference's) runs in the library's deterministic mode, in which ``--seed`` fixes the run to the bit.
``GRAPHPOPE_FULL_INFERENCE=1`` adds, behind the test pass, the accuracy of the trained model on the graph itself -- every node, every
neighbour, no sampling (``SAGE.inference``) -- as a ``full_val_acc`` / ``full_test_acc`` line; nothing else changes.
``GRAPHPOPE_SAGE_AGGR=add|max`` (default ``mean``, the reference's) selects the aggregator of every SAGEConv (``SAGE(aggr=...)``).
``GRAPHPOPE_MODEL=gcn`` (default ``sage``: exactly the run above) trains a full-batch ``graphpope_amd.gcn.GCN`` on the same tensor instead:
one step per epoch over the whole graph, the loss on the training rows, the same optimiser, scheduler and early stopping; ``--dropout`` IS
handed to that model, ``--batch_size`` is unused, and ``--n_gpus`` must be 1.  There ``GRAPHPOPE_GCN_LAYER=gat`` (default ``gcn``) builds
``graphpope_amd.gat.GAT`` with ``GRAPHPOPE_GAT_HEADS`` heads (default 8, a divisor of ``--hidden_layer_size``) in its place, and
``GRAPHPOPE_GCN_LAYER=gatv2`` ``graphpope_amd.gatv2.GATv2`` (per-edge dynamic attention) under the same heads rule.

``--n_gpus N`` with N > 1 is Lightning's ``Trainer(gpus=N, accelerator='ddp')`` (main.py:285-290), data-parallel training over N
processes (graphpope_amd.parallel).  Without a launcher (``WORLD_SIZE`` unset) this process only starts the N ranks
(:func:`ddp_launch_command`) and waits for them; under one it is a rank, and ``WORLD_SIZE`` must equal N.
``GRAPHPOPE_DDP_BACKEND=nccl|gloo`` (default ``nccl``: RCCL, one device per rank) picks the backend of the ranks' process group.
"""
from __future__ import annotations

import argparse
import builtins
import os
import os.path as osp
import random
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

from . import parallel, synth
from .optim import Adam
from . import engine
from .sage import SAGE, EvalMetrics, IndexedFeatures, cross_entropy, deterministic
from .sampler import NeighborSampler
from .train import SageEvalStep, SageTrainStep
from .utils import Graphpope


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description='GraphPOPE')
    # Pope arguments
    parser.add_argument('--dataset', type=str, default='flickr')  # flickr, pubmed
    parser.add_argument('--embedding_space', type=str, default='geodesic')  # node2vec, geodesic, baseline
    parser.add_argument('--sampling_method', type=str, default='degree_centrality')
    parser.add_argument('--num_anchor_nodes', type=int, default=2)
    parser.add_argument('--distance_function', type=str, default=None)  # distance, similarity, euclidean
    parser.add_argument('--num_workers', type=int, default=6)
    # Additional hyperparams
    parser.add_argument('--dropout', type=float, default=0.5)
    parser.add_argument('--lr', type=float, default=0.001)
    parser.add_argument('--num_layers', type=int, default=3)
    parser.add_argument('--hidden_layer_size', type=int, default=256)
    parser.add_argument('--batch_size', type=int, default=1550)
    parser.add_argument('--epochs', type=int, default=300)
    parser.add_argument('--seed', type=int, default=42)
    parser.add_argument('--wandb_logging', type=bool, default=False)
    parser.add_argument('--n_gpus', type=int, default=1)
    return parser


class GraphData:
    """The attributes of a PyG ``Data`` object this path touches."""

    def __init__(self, x, y, edge_index, train_mask, val_mask, test_mask):
        self.x, self.y, self.edge_index = x, y, edge_index
        self.train_mask, self.val_mask, self.test_mask = train_mask, val_mask, test_mask
        self.num_nodes = int(x.shape[0])


def seed_everything(seed: int):
    random.seed(seed)
    np.random.seed(seed)                     # the anchor draw uses this global legacy stream (utils.py:22-24)
    torch.manual_seed(seed)


def load_dataset(name: str, data_dir: str) -> tuple[GraphData, int]:
    """(data, num_classes): real arrays if ``<data_dir>/<name>.npz`` exists, else a synthetic graph of that shape."""
    classes = 7 if name == 'flickr' else 3                                   # main.py:81-83, 141-143
    path = osp.join(data_dir, f'{name}.npz')
    if osp.exists(path):
        z = np.load(path)
        t = {k: torch.as_tensor(z[k]) for k in z.files}
        return GraphData(t['x'].float(), t['y'].long(), t['edge_index'].long(), t['train_mask'].bool(),
                         t['val_mask'].bool(), t['test_mask'].bool()), classes
    ei, n = synth.flickr_like() if name == 'flickr' else synth.pubmed_like()
    g = torch.Generator().manual_seed(0)
    x = torch.rand(n, 500, generator=g)                                     # 500 features: main.py:77-79, 137-139
    y = torch.randint(0, classes, (n,), generator=g)
    split = torch.rand(n, generator=g)
    return GraphData(x, y, torch.as_tensor(ei), split < 0.5, (split >= 0.5) & (split < 0.75), split >= 0.75), classes


def _epoch_order(node_idx, shuffle, gen):
    return node_idx[torch.randperm(node_idx.numel(), device=node_idx.device, generator=gen)] if shuffle else node_idx


def ddp_launch_command(argv, n: int) -> list:
    """What ``--n_gpus n`` without a launcher starts: torch's elastic launcher with n ranks of this module on this node, same flags."""
    return [sys.executable, '-m', 'torch.distributed.run', '--standalone', '--nnodes=1', '--nproc-per-node', str(int(n)),
            '-m', 'graphpope_amd.main', *[str(a) for a in argv]]


def ddp_world(n_gpus: int, environ) -> int:
    """Ranks of the process group this process is to join: 0 = none (a plain single-process run), -1 = none yet, this process is the
    parent that starts them.  With WORLD_SIZE set (a launcher started us) the process is one rank, and WORLD_SIZE must be --n_gpus:
    anything else used to train the same model WORLD_SIZE times over.  Needs no GPU."""
    world = environ.get('WORLD_SIZE')
    if world is None:
        return -1 if n_gpus > 1 else 0
    if int(world) != n_gpus:
        raise ValueError(f"--n_gpus {n_gpus} under a launcher with WORLD_SIZE={world}: the two must agree")
    return n_gpus if n_gpus > 1 else 0


def ddp_backend_from_env(environ=os.environ) -> str:
    """GRAPHPOPE_DDP_BACKEND: 'nccl' (RCCL, the default) or 'gloo'; anything else is a ValueError."""
    backend = environ.get('GRAPHPOPE_DDP_BACKEND', 'nccl')
    if backend not in ('nccl', 'gloo'):
        raise ValueError(f"GRAPHPOPE_DDP_BACKEND={backend!r}: expected nccl or gloo")
    return backend


def ddp_device_index(backend: str, world: int, local_rank: int, device_count: int) -> int:
    """The device of a rank: LOCAL_RANK modulo the device count, as utils._device picks it.  RCCL refuses two ranks on one device, so
    fewer devices than ranks is an error there, raised before the group is created."""
    if device_count < 1:
        raise RuntimeError("graphpope_amd.main: no GPU (there is no CPU fallback)")
    if backend == 'nccl' and device_count < world:
        raise RuntimeError(f"--n_gpus {world} with {device_count} device(s): the nccl backend (RCCL) cannot put two ranks on one device; "
                           "GRAPHPOPE_DDP_BACKEND=gloo can (slowly)")
    return local_rank % device_count


def _launch_ranks(argv, n: int):
    """The parent of a data-parallel run: n fresh child processes (never exec), no GPU touched here.  Rank 0's lines pass through; the
    run's value is the test_acc it printed.  A failing child fails the run."""
    proc = subprocess.Popen(ddp_launch_command(argv, n), stdout=subprocess.PIPE, text=True)
    te_acc = None
    try:
        for line in proc.stdout:
            sys.stdout.write(line)
            sys.stdout.flush()
            if line.startswith('test_acc '):
                te_acc = float(line.split()[1])
        code = proc.wait()
    finally:
        if proc.poll() is None:                               # interrupted: the launcher takes its ranks down with it
            proc.terminate()
            proc.wait()
    if code != 0:
        raise RuntimeError(f"data-parallel run failed: the launcher of the {n} ranks returned {code}")
    if te_acc is None:
        raise RuntimeError("data-parallel run: rank 0 printed no test_acc line")
    return te_acc


def _reduced(metrics, group):
    metrics.all_reduce(group)
    mean_loss, acc, rows = metrics.read()
    return (mean_loss, acc) if rows else (0.0, 0.0)


def _run_epoch(model, feats, labels, sampler, node_idx, args, gen, epoch, opt=None, trainer=None, evaluator=None, group=None,
               bucket=None):
    """One pass over node_idx.  Everything stays on the device: the fan-out sampler (main.py:100-116), the feature
    gather of convert_batch (main.py:118-123), the model, the optimiser; loss / accuracy are accumulated on the
    device and read once per epoch.  Full training batches go through `trainer` (graphpope_amd.train.SageTrainStep:
    sampled with device extents, the whole step replayed as a HIP graph, nothing read back -- in its epoch mode the step
    also takes its seeds from the epoch's shuffled order and gathers their labels itself, so a training step has no
    per-batch input at all); the last, shorter batch of an epoch takes the eager path below.  A training pass adds its loss and
    accuracy with one launch per step (sage.EvalMetrics).  An evaluation pass of at least one full batch goes through `evaluator`
    (graphpope_amd.train.SageEvalStep: the forward-only step, replayed); without one it takes the eager path, batch by batch.
    `group` (data-parallel run): node_idx is this rank's share, a training pass takes it in the order given (parallel.partition has
    shuffled it) and averages the tail batch's gradients through `bucket`, and the pass's three metric words are summed over the ranks."""
    train = opt is not None
    if not train and evaluator is not None and node_idx.numel() >= args.batch_size:
        res = evaluator.run_pass(node_idx, labels, (args.seed << 20) + (epoch << 10))       # batch b: the eager loop's seed + b
        return res if group is None else _reduced(evaluator.metrics, group)
    model.train(train)
    dev = feats.device
    metrics = EvalMetrics(dev) if train or group is not None else None
    tot_loss = torch.zeros((), device=dev)
    tot_correct = torch.zeros((), device=dev, dtype=torch.int64)
    tot = 0
    order = node_idx if group is not None else _epoch_order(node_idx, train, gen)        # NeighborSampler(node_idx, shuffle=train)
    use_trainer = train and trainer is not None
    if use_trainer:
        trainer.set_epoch(order, labels)
    for b, lo in enumerate(range(0, order.numel(), args.batch_size)):
        seeds = order[lo:lo + args.batch_size]
        if use_trainer and seeds.numel() == args.batch_size:
            trainer.step_epoch()                                                         # seeds = order[lo : lo + batch_size], y gathered on the way
            y_hat, y = trainer.logits, trainer.y
        else:
            y = labels.index_select(0, seeds)                                            # Batch.y = data.y[n_id[:batch_size]]
            n_id, adjs = sampler.sample(seeds, seed=(args.seed << 20) + (epoch << 10) + b)   # NeighborSampler(sizes=[25, 10])
            x = IndexedFeatures(feats, n_id)                                             # Batch.x = data.x[n_id], never materialised
            with torch.set_grad_enabled(train):
                y_hat = model(x, adjs)
                loss = cross_entropy(y_hat, y)                                           # main.py:216 F.cross_entropy
            if train:
                for p in model.parameters():
                    p.grad = None
                loss.backward()
                if bucket is not None:
                    bucket.sync(group)                                                   # the mean over the ranks, before the clip
                opt.step()                                                               # clips too: Adam(max_grad_norm=0.5) below
                if trainer is not None:
                    trainer.state.advance()                                              # the optimiser reads its step count from the trainer's device word
        if metrics is not None:
            metrics.update(y_hat, y)                                                     # main.py:216-217: loss sum, correct and rows in one launch
        else:
            tot_loss += loss.detach() * seeds.numel()
            tot_correct += (y_hat.argmax(-1) == y).sum()
            tot += seeds.numel()
    if group is not None:
        return _reduced(metrics, group)
    if train:
        mean_loss, acc, rows = metrics.read()
        return (mean_loss, acc) if rows else (0.0, 0.0)
    return float(tot_loss) / max(tot, 1), int(tot_correct) / max(tot, 1)


def _make_evaluator(model, feats, batch_size, sampler, max_nodes):
    """The one SageEvalStep the validation and the test pass share, its buffers sized for the larger split -- or None, and both take the
    eager path of :func:`_run_epoch`: with GRAPHPOPE_EVAL_STEP=eager, or when no split holds a full batch."""
    if os.environ.get('GRAPHPOPE_EVAL_STEP', 'graph') == 'eager' or max_nodes < batch_size:
        return None
    return SageEvalStep(model, feats, batch_size, sampler, max_nodes=max_nodes)


def _full_accuracy(model, feats, labels, adj_t, hops, splits):
    """Accuracy of the model's exact full-graph prediction (SAGE.inference: all neighbours, running BatchNorm statistics) on each index
    set of `splits`; the depth is the sampler's, as in training (main.py:204: the loop runs over the sampled adjs)."""
    logits = model.inference(feats, adj_t, hops=hops)
    accs = []
    for nodes in splits:
        metrics = EvalMetrics(feats.device)
        if nodes.numel():
            metrics.update(logits.index_select(0, nodes), labels.index_select(0, nodes))
        accs.append(metrics.read()[1])
    return accs


def sage_aggr_from_env() -> str:
    """GRAPHPOPE_SAGE_AGGR: 'mean' (the default), 'add' or 'max'; anything else is a ValueError, raised before the GPU is touched."""
    aggr = os.environ.get('GRAPHPOPE_SAGE_AGGR', 'mean')
    if aggr not in ('mean', 'add', 'max'):
        raise ValueError(f"GRAPHPOPE_SAGE_AGGR={aggr!r}: expected mean, add or max")
    return aggr


def model_from_env(environ=os.environ) -> str:
    """GRAPHPOPE_MODEL: 'sage' (the default, the reference's sampled GraphSAGE) or 'gcn' (a full-batch GCN, graphpope_amd.gcn); anything
    else is a ValueError, raised before the GPU is touched."""
    model = environ.get('GRAPHPOPE_MODEL', 'sage')
    if model not in ('sage', 'gcn'):
        raise ValueError(f"GRAPHPOPE_MODEL={model!r}: expected sage or gcn")
    return model


def gcn_layer_from_env(hidden: int, environ=os.environ):
    """(layer, heads) of the full-batch trainer behind GRAPHPOPE_MODEL=gcn.  GRAPHPOPE_GCN_LAYER: 'gcn' (the default: gcn.GCN), 'gat'
    (gat.GAT with GRAPHPOPE_GAT_HEADS heads, default 8, which must divide --hidden_layer_size) or 'gatv2' (gatv2.GATv2, the same heads
    rule); anything else is a ValueError, raised before the GPU is touched."""
    layer = environ.get('GRAPHPOPE_GCN_LAYER', 'gcn')
    if layer not in ('gcn', 'gat', 'gatv2'):
        raise ValueError(f"GRAPHPOPE_GCN_LAYER={layer!r}: expected gcn, gat or gatv2")
    if layer == 'gcn':
        return layer, 0
    raw = environ.get('GRAPHPOPE_GAT_HEADS', '8')
    try:
        heads = int(raw)
    except ValueError:
        heads = 0
    if heads < 1 or hidden % heads:
        raise ValueError(f"GRAPHPOPE_GAT_HEADS={raw!r}: expected a positive integer that divides --hidden_layer_size {hidden}")
    return layer, heads


def main(argv=None):
    """GRAPHPOPE_DETERMINISTIC=1: the run in the library's deterministic mode (sage.set_deterministic), so that a seed fixes the
    weights it ends with; the previous mode is restored on the way out."""
    args = build_parser().parse_args(argv)
    sage_aggr_from_env()
    if model_from_env() == 'gcn' and args.n_gpus > 1:
        raise ValueError(f"GRAPHPOPE_MODEL=gcn trains full-batch on one device: --n_gpus {args.n_gpus} is not supported")
    if model_from_env() == 'gcn':
        gcn_layer_from_env(args.hidden_layer_size)            # ValueError before the GPU is touched
    world = ddp_world(args.n_gpus, os.environ)                # ValueError before the GPU is touched
    if world < 0:                                             # --n_gpus N > 1 and no launcher: start the N ranks, wait, pass on rank 0's result
        ddp_backend_from_env()
        return _launch_ranks(sys.argv[1:] if argv is None else argv, args.n_gpus)
    if os.environ.get('GRAPHPOPE_DETERMINISTIC', '0') != '1':
        return _main(args, world)
    with deterministic(True):
        return _main(args, world)


def _init_rank(world: int):
    """One rank of a data-parallel run: its device, then the process group (before Graphpope(), whose geodesic branch shards its anchors
    over the ranks of an initialised group)."""
    import torch.distributed as dist
    backend = ddp_backend_from_env()
    index = ddp_device_index(backend, world, int(os.environ.get('LOCAL_RANK', 0)), torch.cuda.device_count())
    dev = torch.device('cuda', index)
    torch.cuda.set_device(dev)
    if backend == 'nccl':
        dist.init_process_group(backend, device_id=dev)
    else:
        dist.init_process_group(backend)
    if dist.get_world_size() != world:
        raise RuntimeError(f"process group of {dist.get_world_size()} ranks, --n_gpus {world}")
    return dev, dist.group.WORLD, dist.get_rank()


def _main(args, world: int = 0):
    """world 0: the single-process run.  world > 1: this process is one rank of a data-parallel run (graphpope_amd.parallel) -- the
    training nodes are split as Lightning's DistributedSampler splits them, the gradients averaged in one bucket before the clip, the
    metric words of every pass summed over the ranks, so all ranks feed the same val_loss to the scheduler and the same val_acc to the
    early-stopping counter and stop together; only rank 0 prints."""
    if world > 1:
        dev, group, rank = _init_rank(world)
        try:
            return _train(args, dev, group, world, rank)
        finally:
            torch.distributed.destroy_process_group()
    dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0)))
    torch.cuda.set_device(dev)
    return _train(args, dev)


def _train(args, dev, group=None, world: int = 1, rank: int = 0):
    print = builtins.print if rank == 0 else (lambda *a, **k: None)
    print(args)
    seed_everything(args.seed)
    data_dir = os.environ.get('GRAPHPOPE_DATA_DIR', osp.join(os.getcwd(), 'data'))
    data, num_classes = load_dataset(args.dataset, data_dir)
    if args.embedding_space != 'baseline':                                               # main.py:94-98
        data.x = Graphpope(data=data, dataset=args.dataset, embedding_space=args.embedding_space,
                           sampling_method=args.sampling_method, num_anchor_nodes=args.num_anchor_nodes,
                           distance_function=args.distance_function, num_workers=args.num_workers)
    in_channels = int(500 + args.num_anchor_nodes)                                       # main.py:77-79 (hard-coded 500 + K)
    if model_from_env() == 'gcn':
        return _train_gcn(args, dev, data, in_channels, num_classes, print)
    model = SAGE(in_channels, num_classes, args.hidden_layer_size, args.num_layers, aggr=sage_aggr_from_env()).to(dev)   # dropout NOT passed: main.py:272
    # main.py:244 torch.optim.Adam rule in one launch per step, with gradient_clip_val=0.5 of both Trainer(...) calls (main.py:285-290) inside it
    opt = Adam(model.parameters(), lr=args.lr, max_grad_norm=0.5)
    if group is not None:
        parallel.broadcast_parameters(model, group)           # equal already by the shared seed; made so anyway
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt)                              # monitors val_loss
    # HBM-resident training data: features (+ POPE columns), labels, and adj_t as a device CSR whose row v lists the nodes v
    # aggregates from (main.py:84 ToSparseTensor: the transposed adjacency; the same CSR for the symmetric Flickr / PubMed)
    feats, labels = data.x.to(dev, torch.float32).contiguous(), data.y.to(dev)
    adj_t = engine.build_csr(data.edge_index.flip(0).contiguous().to(dev), data.num_nodes)
    sampler = NeighborSampler(adj_t.rowptr, adj_t.col, data.num_nodes, sizes=(25, 10))
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    idx = {k: torch.nonzero(getattr(data, f'{k}_mask'), as_tuple=False).flatten().to(dev) for k in ('train', 'val', 'test')}
    best, bad = -1.0, 0
    torch.autograd.set_multithreading_enabled(False)          # backward in the calling thread: the step is launch-bound on the host
    trainer = bucket = None
    whole = (idx['val'], idx['test'])
    if group is not None:                                     # evaluation: node_idx[rank::world], every node counted once
        idx['val'], idx['test'] = (parallel.partition_eval(idx[k], world, rank) for k in ('val', 'test'))
    if os.environ.get('GRAPHPOPE_TRAIN_STEP', 'graph') != 'eager' and -(-idx['train'].numel() // world) >= args.batch_size:
        trainer = SageTrainStep(model, opt, feats, args.batch_size, sampler=sampler, clip=None, seed=args.seed, group=group)   # the clip is the optimiser's
    if group is not None:                                     # the eager tail batch shares the step's bucket
        bucket = trainer.bucket if trainer is not None else parallel.GradBucket(model.parameters())
    evaluator = _make_evaluator(model, feats, args.batch_size, sampler, max(idx['val'].numel(), idx['test'].numel()))
    for epoch in range(args.epochs):
        order = idx['train'] if group is None else parallel.partition(idx['train'], world, rank, True, args.seed, epoch)
        tr_loss, tr_acc = _run_epoch(model, feats, labels, sampler, order, args, gen, epoch, opt, trainer, group=group, bucket=bucket)
        if group is not None:
            parallel.broadcast_buffers(model, group)          # BatchNorm statistics are per rank while training: evaluate rank 0's
        va_loss, va_acc = _run_epoch(model, feats, labels, sampler, idx['val'], args, gen, epoch, evaluator=evaluator, group=group)
        sched.step(va_loss)
        print(f'epoch {epoch}: train_loss {tr_loss:.4f} train_acc {tr_acc:.4f} val_loss {va_loss:.4f} val_acc {va_acc:.4f}')
        if va_acc > best:
            best, bad = va_acc, 0
        else:
            bad += 1
            if bad >= 20:                                                                # EarlyStopping(val_acc, patience=20)
                break
    if group is not None:
        parallel.broadcast_buffers(model, group)
    _, te_acc = _run_epoch(model, feats, labels, sampler, idx['test'], args, gen, args.epochs, evaluator=evaluator, group=group)
    print(f'test_acc {te_acc:.4f}')
    if os.environ.get('GRAPHPOPE_FULL_INFERENCE', '0') == '1':
        full = _full_accuracy(model, feats, labels, adj_t, len(sampler.sizes), whole)
        print(f'full_val_acc {full[0]:.4f} full_test_acc {full[1]:.4f}')
    if group is not None:
        parallel.assert_same_parameters(model, group)         # every rank holds rank 0's weights, or the run fails
    return te_acc


def _train_gcn(args, dev, data, in_channels, num_classes, print):
    """GRAPHPOPE_MODEL=gcn: full-batch training of gcn.GCN on ``x (+) POPE``, one step per epoch over the whole graph.  The loss is
    taken on the training rows; optimiser, clipping, scheduler and early stopping are the sampled loop's (main.py:243-255, 279-290);
    validation and test run the same forward in eval mode."""
    from .gcn import GCN, GraphAdj
    print(f'GRAPHPOPE_MODEL=gcn: full-batch training, --batch_size {args.batch_size} is unused')
    layer, heads = gcn_layer_from_env(args.hidden_layer_size)
    if layer == 'gat':
        from .gat import GAT
        model = GAT(in_channels, args.hidden_layer_size, num_classes, args.num_layers, heads=heads, dropout=args.dropout).to(dev)
    elif layer == 'gatv2':
        from .gatv2 import GATv2
        model = GATv2(in_channels, args.hidden_layer_size, num_classes, args.num_layers, heads=heads, dropout=args.dropout).to(dev)
    else:
        model = GCN(in_channels, args.hidden_layer_size, num_classes, args.num_layers, dropout=args.dropout).to(dev)
    opt = Adam(model.parameters(), lr=args.lr, max_grad_norm=0.5)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt)
    feats, labels = data.x.to(dev, torch.float32).contiguous(), data.y.to(dev)
    adj = GraphAdj(data.edge_index.to(dev), data.num_nodes)
    idx = {k: torch.nonzero(getattr(data, f'{k}_mask'), as_tuple=False).flatten().to(dev) for k in ('train', 'val', 'test')}
    y = {k: labels.index_select(0, v) for k, v in idx.items()}
    torch.autograd.set_multithreading_enabled(False)

    def evaluate(logits, split):
        metrics = EvalMetrics(dev)
        if idx[split].numel():
            metrics.update(logits.index_select(0, idx[split]), y[split])
        mean_loss, acc, rows = metrics.read()
        return (mean_loss, acc) if rows else (0.0, 0.0)

    best, bad = -1.0, 0
    for epoch in range(args.epochs):
        model.train(True)
        logits = model(feats, adj)
        loss = cross_entropy(logits.index_select(0, idx['train']), y['train'])
        for p in model.parameters():
            p.grad = None
        loss.backward()
        opt.step()
        tr_loss, tr_acc = evaluate(logits.detach(), 'train')
        model.train(False)
        with torch.no_grad():
            logits = model(feats, adj)
        va_loss, va_acc = evaluate(logits, 'val')
        sched.step(va_loss)
        print(f'epoch {epoch}: train_loss {tr_loss:.4f} train_acc {tr_acc:.4f} val_loss {va_loss:.4f} val_acc {va_acc:.4f}')
        if va_acc > best:
            best, bad = va_acc, 0
        else:
            bad += 1
            if bad >= 20:
                break
    model.train(False)
    with torch.no_grad():
        _, te_acc = evaluate(model(feats, adj), 'test')
    print(f'test_acc {te_acc:.4f}')
    return te_acc


if __name__ == "__main__":
    main()
