"""Generate the node2vec table ``attach_node2vec`` loads: the drop-in for /root/reference/generate_node2vec_embedding.py.

    python -m graphpope_amd.generate_node2vec_embedding --dataset pubmed [--epochs 5]

Same model and hyper-parameters as the reference's script (generate_node2vec_embedding.py:23-25: embedding_dim 128, walk_length 20,
context_size 10, walks_per_node 10, num_negative_samples 1, p 1, q 1, sparse True), each also a flag; the same two printed lines; the
table is saved as a CPU float32 ``[N, D]`` tensor to ``utils.NODE2VEC_DIR/{dataset.lower()}_node2vec.pt`` (``--out`` overrides).

=====================  ======================  ==========================================================================
``--p`` / ``--q``      model                   walks
=====================  ======================  ==========================================================================
both 1 (the default)   Node2Vec                uniform first-order walks (pope_n2v_walks): the reference-default run
any other finite > 0   SecondOrderNode2Vec     second-order walks on the canonical CSR (pope_n2v_walks_biased): ``q > 1`` keeps
                                               a walk near its previous node (BFS-like), ``q < 1`` sends it outwards (DFS-like),
                                               a large ``p`` makes it unlikely to step straight back
=====================  ======================  ==========================================================================

The reference's script never trains: it constructs the model, calls ``model()`` and saves the initial N(0, 1) table (SURVEY.md §8d
config 3).  ``--epochs 0``, the default, does exactly that: the file is bit-identical to ``torch.manual_seed(seed);
torch.nn.Embedding(N, D).weight`` on the CPU.  ``--epochs E`` trains first (``Node2Vec.fit``: walks, skip-gram loss and SparseAdam on
the GPU).  ``--eval`` adds PyG's ``Node2Vec.test`` on the dataset's train / test split (``Node2Vec.test_nodes``, ``max_iter=150``):
one line for the untrained table with no epochs, else ``epoch e: loss L acc A`` per epoch; the saved table is the same.  The graph comes from ``main.load_dataset``: ``<--data_dir>/<dataset>.npz`` if present, else a synthetic graph of the
dataset's shape.  Flags are parsed in ``main()``, not at import.
"""
from __future__ import annotations

import argparse
import os
import os.path as osp

import torch

from . import utils
from .node2vec import Node2Vec, SecondOrderNode2Vec


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description='GraphPOPE node2vec embedding generator')
    parser.add_argument('--dataset', type=str, default='PubMed')   # generate_node2vec_embedding.py:16; flickr: the commented-out block
    parser.add_argument('--data_dir', type=str, default=None)
    parser.add_argument('--out', type=str, default=None)
    # the reference's eight hyper-parameters (generate_node2vec_embedding.py:23-25)
    parser.add_argument('--embedding_dim', type=int, default=128)
    parser.add_argument('--walk_length', type=int, default=20)
    parser.add_argument('--context_size', type=int, default=10)
    parser.add_argument('--walks_per_node', type=int, default=10)
    parser.add_argument('--num_negative_samples', type=int, default=1)
    parser.add_argument('--p', type=float, default=1)
    parser.add_argument('--q', type=float, default=1)
    parser.add_argument('--sparse', type=lambda s: s.lower() not in ('0', 'false', 'no'), default=True)
    # training: off by default, as in the reference
    parser.add_argument('--epochs', type=int, default=0)
    parser.add_argument('--batch_size', type=int, default=128)
    parser.add_argument('--lr', type=float, default=0.01)
    parser.add_argument('--seed', type=int, default=42)
    # PyG's Node2Vec.test on the dataset's split, before training and after every epoch: off by default, as the reference prints no accuracy
    parser.add_argument('--eval', action='store_true', default=False)
    return parser


def main(argv=None):
    """GRAPHPOPE_DETERMINISTIC=1 (as for graphpope_amd.main): the run in the library's deterministic mode, in which ``--seed`` fixes
    the trained table to the bit; the previous mode is restored on the way out."""
    from .sage import deterministic
    args = build_parser().parse_args(argv)
    if os.environ.get('GRAPHPOPE_DETERMINISTIC', '0') != '1':
        return _main(args)
    with deterministic(True):
        return _main(args)


def _main(args):
    from .main import load_dataset, seed_everything
    seed_everything(args.seed)
    dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0)))
    torch.cuda.set_device(dev)
    data_dir = args.data_dir or os.environ.get('GRAPHPOPE_DATA_DIR', osp.join(os.getcwd(), 'data'))
    name = args.dataset.lower()
    data, _ = load_dataset(name, data_dir)
    print('data loaded in!')
    model_class = Node2Vec if args.p == 1 and args.q == 1 else SecondOrderNode2Vec
    model = model_class(data.edge_index.to(dev), embedding_dim=args.embedding_dim, walk_length=args.walk_length,
                        context_size=args.context_size, walks_per_node=args.walks_per_node,
                        num_negative_samples=args.num_negative_samples, p=args.p, q=args.q, num_nodes=data.num_nodes, sparse=args.sparse)
    if args.eval:
        train_ids, test_ids = (mask.nonzero().reshape(-1) for mask in (data.train_mask, data.test_mask))

        def accuracy():
            return model.test_nodes(train_ids, test_ids, data.y, max_iter=150)      # 150: the PyG node2vec example's value

        if args.epochs <= 0:
            print(f'untrained: acc {accuracy():.4f}')
        model.fit(args.epochs, batch_size=args.batch_size, lr=args.lr, seed=args.seed,
                  on_epoch=lambda epoch, loss: print(f'epoch {epoch}: loss {loss:.4f} acc {accuracy():.4f}'))
    elif args.epochs > 0:
        for epoch, loss in enumerate(model.fit(args.epochs, batch_size=args.batch_size, lr=args.lr, seed=args.seed)):
            print(f'epoch {epoch}: loss {loss:.4f}')
    embeddings = model(torch.arange(data.num_nodes, device=dev)).detach().to('cpu', torch.float32).contiguous()
    save_path = args.out or osp.join(utils.NODE2VEC_DIR, f'{name}_node2vec.pt')
    os.makedirs(osp.dirname(osp.abspath(save_path)), exist_ok=True)
    torch.save(embeddings, save_path)
    print(f'saved node2vec embedding as {name}_node2vec.pt!')
    return save_path


if __name__ == "__main__":
    main()
