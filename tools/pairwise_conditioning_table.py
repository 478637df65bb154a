#!/usr/bin/env python3
"""Scaled error of the node2vec-space path on the off-centre tables of tests/pairwise_cases.py, one row per case and
kernel path (GPU box):  python tools/pairwise_conditioning_table.py [--lib other/libgraphpope_hip.so] > table.txt

euclidean: max |out - scale64(ref64)| and the ratio d2 / (|x|^2 + |a|^2) of the worst output; then, for every candidate
threshold, the largest error among the outputs whose ratio lies at or above it -- the outputs a kernel with that
threshold would still take from the float32 expansion.  Cosine metrics: the kernel's and the oracle's deviation from
float64 and their quotient (the test bounds the kernel by 2 x the oracle's).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of the library")
    args = ap.parse_args()
    from graphpope_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    import torch
    import pairwise_cases as pc
    from graphpope_amd import engine
    from oracle import oracle
    dev = engine.require_gpu()
    lib = _lib.load()
    candidates = [2.0 ** -e for e in range(7, 0, -1)]
    above = {(kern, g): 0.0 for kern in range(4) for g in candidates}         # max error among outputs with ratio >= g
    worst_cos = {}
    print(f"# library: {os.path.relpath(_lib.LIB_PATH, ROOT)}; CANCEL_RATIO of the cases: {pc.CANCEL_RATIO:g} "
          "('below thr %' is the share of non-coincident pairs below THAT value, whatever the library's threshold is)")
    print(f"# {'case':<36} {'kernel':>6} {'euclid err':>11} {'ratio@worst':>11} {'below thr %':>11} "
          f"{'dist err':>9} {'dist ref':>9} {'quot':>5} {'sim err':>9} {'sim ref':>9} {'quot':>5}")
    for c in pc.CASES:
        i = pc.inputs(c.name)
        emb_d = torch.as_tensor(np.array(i.emb), device=dev)         # a copy: the shared inputs are read-only arrays
        rows_d = torch.as_tensor(i.emb[i.anchors], device=dev)
        x_d = torch.as_tensor(pc.features(c.n, 8), device=dev)
        ratio = pc.ratio64(i.emb, i.anchors)
        below = 100.0 * float((ratio[~pc.coincident(i.emb, i.anchors)] < pc.CANCEL_RATIO).mean())
        ref_dev = {fn: float(np.abs(oracle.minmax_scale_columns(oracle.pairwise(i.emb, i.emb[i.anchors], fn)) - pc.want64(c.name, fn)).max())
                   for fn in ("distance", "similarity")}
        for kern in ((0, 1, 2, 3) if c.d <= 128 and c.d % 4 == 0 else (0,)):
            lib.pope_debug_set(_lib.KNOB_PAIRWISE_KERNEL, kern)
            try:
                err = {}
                for fn in pc.FNS:
                    a = engine.pairwise_features(x_d, emb_d, i.anchors, fn).cpu().numpy()[:, 8:]
                    b = engine.pairwise_features(x_d, emb_d, None, fn, anchor_embeddings=rows_d).cpu().numpy()[:, 8:]
                    err[fn] = np.maximum(np.abs(a - pc.want64(c.name, fn)), np.abs(b - pc.want64(c.name, fn)))
            finally:
                lib.pope_debug_set(_lib.KNOB_PAIRWISE_KERNEL, 0)
            e = err["euclidean"]
            at = np.unravel_index(int(np.nanargmax(e)), e.shape)
            for g in candidates:
                sel = ratio >= g
                if sel.any():
                    above[kern, g] = max(above[kern, g], float(e[sel].max()))
            cells = []
            for fn in ("distance", "similarity"):
                m = float(np.nanmax(err[fn])) if np.isfinite(err[fn]).all() else float("nan")
                q = m / ref_dev[fn]
                cells.append(f"{m:9.2e} {ref_dev[fn]:9.2e} {q:5.2f}")
                if ref_dev[fn] > 5e-6:                                    # below that the test's bound is the flat 1e-5
                    key = (kern, fn)
                    if key not in worst_cos or q > worst_cos[key][0]:
                        worst_cos[key] = (q, c.name)
            print(f"  {c.name:<36} {kern:>6} {float(e[at]):11.2e} {float(ratio[at]):11.4f} {below:11.2f} {cells[0]} {cells[1]}")
    print("#\n# largest euclidean error among the outputs with d2 / norms >= threshold (all cases), per kernel path")
    print("# threshold " + " ".join(f"{'kernel ' + str(kern):>10}" for kern in range(4)))
    for g in candidates:
        print(f"  2^-{int(round(-np.log2(g)))} = {g:<8.5f}".ljust(12) + " ".join(f"{above[kern, g]:10.2e}" for kern in range(4)))
    print("#\n# largest kernel / oracle quotient of the cosine deviations (cases whose oracle deviation exceeds 5e-6)")
    for (kern, fn), (q, name) in sorted(worst_cos.items()):
        print(f"  kernel {kern} {fn:<10} {q:5.2f}  {name}")


if __name__ == "__main__":
    main()
