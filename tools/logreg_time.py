#!/usr/bin/env python3
"""Time ``Node2Vec.test`` on the GPU (graphpope_amd.logreg over pope_logreg_loss_grad / pope_logreg_predict) at the Flickr-shaped
table (N = 89 250, D = 128, 7 classes) and the PubMed-shaped one (N = 19 717, 3 classes), with ``main.load_dataset``'s labels and
train / test split.  Two tables per shape: ``untrained``, the N(0, 1) table ``torch.nn.Embedding`` starts from (what the reference's
script saves), and ``blobs``, the same table with a class mean of 0.2 per coordinate added, so that the fit has something to find.
Per shape, in one child process under a time limit:

    objective    ms per pope_logreg_loss_grad call on the training rows through ids: HIP events around blocks of --calls calls,
                 --reps blocks, after --warmup calls; the bytes of one pass over the selected rows of z over that time
    test_nodes   host clock around one whole fit + score through row ids (ends in a synchronise), with its iteration count, beside
    sklearn      LogisticRegression(max_iter=150).fit(z[train], y[train]).score(z[test], y[test]) on the host, same process, same
                 rows (float64 copy), taken in turns with the above; and whether the two scores are the same float

The first child that fails ends the run.  Prints one JSON object; --out FILE also writes it there (profiles/logreg_times.json)."""
import argparse
import faulthandler
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, MAX_ITER = 128, 150


def gpu_run(name, calls, warmup, reps, time_limit):
    import torch
    from sklearn.linear_model import LogisticRegression
    from graphpope_amd import _lib, engine, logreg
    from graphpope_amd.main import load_dataset
    faulthandler.dump_traceback_later(time_limit, exit=True)
    dev = engine.require_gpu()
    lib = _lib.load()
    data, classes = load_dataset(name, os.path.join(ROOT, "no_such_data_dir"))
    n, y = data.num_nodes, data.y.numpy()
    train, test = (m.nonzero().reshape(-1) for m in (data.train_mask, data.test_mask))
    torch.manual_seed(0)
    base = torch.nn.Embedding(n, D).weight.detach()
    mu = torch.randn(classes, D, generator=torch.Generator().manual_seed(1)) * 0.2
    stat = lambda ts: {"min": min(ts), "median": float(np.median(ts)), "max": max(ts), "all": ts}
    out = {"N": n, "D": D, "classes": classes, "train_rows": int(train.numel()), "test_rows": int(test.numel()), "max_iter": MAX_ITER,
           "calls_per_block": calls, "warmup_calls": warmup, "reps": reps, "device": torch.cuda.get_device_name(0)}

    # one objective evaluation alone
    z = base.to(dev)
    m = int(train.numel())
    ids = train.to(dev)
    y_dev = torch.as_tensor(y[train.numpy()], dtype=torch.int32, device=dev)
    r = 1 if classes == 2 else classes
    p = r * (D + 1)
    w = (0.01 * torch.randn(p, dtype=torch.float64, generator=torch.Generator().manual_seed(2))).to(dev)
    res = torch.empty(1 + p, dtype=torch.float64, device=dev)
    scratch = torch.empty(lib.pope_logreg_scratch_bytes(m, D, classes) // 8, dtype=torch.float64, device=dev)

    def objective():
        _lib.check(lib.pope_logreg_loss_grad(_lib.ptr(z), D, n, _lib.ptr(ids), m, D, _lib.ptr(y_dev), classes, 1, _lib.ptr(w), 1.0 / m,
                                             _lib.ptr(res), _lib.c_void_p(res.data_ptr() + 8), _lib.ptr(scratch), scratch.numel() * 8,
                                             engine._stream()))

    def block_ms(k):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(k):
            objective()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / k

    block_ms(warmup)
    times = [block_ms(calls) for _ in range(reps)]
    assert bool(torch.isfinite(res).all())
    row_bytes = m * D * 4
    out["objective_ms"] = stat(times)
    out["objective_z_bytes_one_pass"] = row_bytes
    out["objective_z_bytes_per_second_one_pass"] = row_bytes / (1e-3 * float(np.median(times)))
    out["scratch_bytes"] = int(scratch.numel() * 8)

    # the whole call beside scikit-learn's
    out["tables"] = {}
    for label in ("untrained", "blobs"):
        table = base if label == "untrained" else base + mu[data.y]
        zd = table.to(dev)
        zh = table.numpy().astype(np.float64)
        tr, te = train.numpy(), test.numpy()
        ours, theirs, last = [], [], {}
        model = logreg.fit(zd, y[tr], ids=train, max_iter=MAX_ITER)               # warm-up, and the iteration count
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fitted = logreg.fit(zd, y[tr], ids=train, max_iter=MAX_ITER)
                last["ours"] = logreg.score(fitted, zd, y[te], ids=test)
            torch.cuda.synchronize()
            ours.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                clf = LogisticRegression(max_iter=MAX_ITER).fit(zh[tr], y[tr])
                last["sklearn"] = clf.score(zh[te], y[te])
            theirs.append(1e3 * (time.perf_counter() - t0))
        out["tables"][label] = {"test_nodes_ms": stat(ours), "sklearn_ms": stat(theirs),
                                "sklearn_over_test_nodes": float(np.median(theirs) / np.median(ours)),
                                "n_iter": int(model.n_iter_[0]), "n_iter_sklearn": int(clf.n_iter_[0]),
                                "accuracy": last["ours"], "accuracy_sklearn": last["sklearn"], "same_float": last["ours"] == last["sklearn"],
                                "max_abs_dcoef": float(np.abs(fitted.coef_ - clf.coef_).max())}
    out["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()
    faulthandler.cancel_dump_traceback_later()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="pubmed,flickr")
    ap.add_argument("--calls", type=int, default=200, help="objective calls per timed block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds one shape's run may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--gpu-run", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.gpu_run:
        print(json.dumps(gpu_run(args.gpu_run, args.calls, args.warmup, args.reps, args.timeout)))
        return
    res = {}
    for name in args.graphs.split(","):
        child = subprocess.run(["timeout", "-k", "10", str(args.timeout + 20), sys.executable, os.path.abspath(__file__), "--gpu-run", name,
                                "--calls", str(args.calls), "--warmup", str(args.warmup), "--reps", str(args.reps),
                                "--timeout", str(args.timeout)], stdout=subprocess.PIPE, text=True)
        if child.returncode != 0:                        # a fault, an abort or the time limit: nothing more is started
            raise SystemExit(f"{name}: the GPU run ended with status {child.returncode}; stopping")
        res[name] = json.loads(child.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
