#!/usr/bin/env python3
"""One SHA-256 of the output bytes per case of the node2vec-space call (GPU box), to compare two builds of the library bit for bit:
    python tools/pairwise_bits.py [path/to/libgraphpope_hip.so] > listing.txt
The cases: every row of tests/pairwise_plan_cases.py whose output stays below 512 MB, under its knob, on that file's table (an anchor
among the table's own rows, two coincident rows), and the off-centre table of tests/pairwise_cases.py at MU_STRADDLE under every knob
value (both sides of the cancellation threshold inside one tile) -- each with the three metrics and both anchor forms, through
engine.pairwise_features (rows with x) or engine.pairwise_embedding.  The outputs are deterministic: one run per build."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from graphpope_amd import _lib  # noqa: E402

if len(sys.argv) > 1:
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    probe = ctypes.CDLL(_lib.LIB_PATH)
    for name in [s for s in _lib.SIGNATURES if not hasattr(probe, s)]:       # a build of an earlier commit: it lacks the newest queries
        del _lib.SIGNATURES[name]
from graphpope_amd import engine  # noqa: E402
import pairwise_cases as pc  # noqa: E402
import pairwise_plan_cases as cases  # noqa: E402

dev = engine.require_gpu()
lib = _lib.load()


def run(tag, emb, anchors, f, has_x, knob):
    n, k = emb.shape[0], len(anchors)
    emb_d = torch.as_tensor(np.array(emb), device=dev)
    rows_d = torch.as_tensor(emb[anchors], device=dev)
    x_d = torch.as_tensor(pc.features(n, f), device=dev) if has_x else None
    lib.pope_debug_set(_lib.KNOB_PAIRWISE_KERNEL, knob)
    try:
        for fn in pc.FNS:
            for form in ("ids", "rows"):
                ids, rows = (anchors, None) if form == "ids" else (None, rows_d)
                if has_x:
                    out = engine.pairwise_features(x_d, emb_d, ids, fn, anchor_embeddings=rows)
                else:
                    wide = torch.zeros((n, f + k), dtype=torch.float32, device=dev)
                    out = engine.pairwise_embedding(emb_d, ids, fn, anchor_embeddings=rows, out=wide, c0=f)
                print("%s knob=%d %s %s %s" % (tag, knob, fn, form, hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()), flush=True)
    finally:
        lib.pope_debug_set(_lib.KNOB_PAIRWISE_KERNEL, 0)


for (n, d, k, f, has_x, by_id, knob) in cases.CASES:
    if n * (f + k) * 4 >= 1 << 29:
        continue
    emb, anchors = cases.inputs(n, d, k)
    run("n=%d d=%d k=%d f=%d x=%d (id=%d)" % (n, d, k, f, has_x, by_id), emb, anchors, f, has_x, knob)
i = pc.inputs("n700_k65_d128_mu%g_straddle" % pc.MU_STRADDLE)
for knob in (0, 1, 2, 3):
    run(i.case.name + " f=8 x=1", i.emb, i.anchors, 8, 1, knob)
    run(i.case.name + " f=3 x=1", i.emb, i.anchors, 3, 1, knob)
