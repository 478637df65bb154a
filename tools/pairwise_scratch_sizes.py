"""The scratch size queries of the node2vec-space call at SCRATCH_SHAPES of tests/pairwise_plan_cases.py, from a library given by path, as
JSON on stdout:
    python tools/pairwise_scratch_sizes.py path/to/libgraphpope_hip.so > tests/golden/pairwise_scratch_sizes.json
tests/test_abi.py compares the library it built with that table, so the table is recorded from a build of the commit whose values are to
be kept, never from the tree under test.  Host logic: needs no GPU."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import pairwise_plan_cases as cases  # noqa: E402

QUERIES = ("pope_pairwise_scratch_bytes", "pope_pairwise_by_id_scratch_bytes")


def sizes(lib, args):
    """Both queries at one (N, K, D), in the order of QUERIES."""
    n, k, d = args
    out = []
    for name in QUERIES:
        fn = getattr(lib, name)
        fn.restype = ctypes.c_size_t
        out.append(fn(ctypes.c_int64(n), ctypes.c_int32(k), ctypes.c_int32(d)))
    return out


if __name__ == "__main__":
    lib = ctypes.CDLL(os.path.abspath(sys.argv[1]))
    rows = [{"args": list(a), "bytes": sizes(lib, a)} for a in cases.SCRATCH_SHAPES]
    print("{\n \"queries\": %s,\n \"rows\": [\n  %s\n ]\n}" % (json.dumps(list(QUERIES)), ",\n  ".join(json.dumps(r) for r in rows)))
