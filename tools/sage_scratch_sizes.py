"""The scratch size queries of the SAGE layer at the shapes of tests/sage_backward_cases.py, from a library given by path, as JSON on stdout:
    python tools/sage_scratch_sizes.py path/to/libgraphpope_hip.so > tests/golden/sage_scratch_sizes.json
tests/test_abi.py compares the library it built with that table, so the table is recorded from a build of the commit whose values are to
be kept, never from the tree under test.  Host logic: needs no GPU."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import sage_backward_cases as cases  # noqa: E402

QUERIES = ("sage_conv_scratch_bytes", "sage_conv_backward_indexed_scratch_bytes", "sage_scatter_mean_det_scratch_bytes",
           "sage_conv_forward_indexed_scratch_bytes")


def sizes(lib, args):
    """The four queries at one (n_src, n_dst, nnz, c_in, c_out), in the order of QUERIES, under the library's current mode."""
    n_src, n_dst, nnz, c_in, c_out = args
    i64, i32 = ctypes.c_int64, ctypes.c_int32
    for name in QUERIES:
        getattr(lib, name).restype = ctypes.c_size_t
    return [lib.sage_conv_scratch_bytes(i64(n_src), i64(n_dst), i64(nnz), i32(c_in), i32(c_out)),
            lib.sage_conv_backward_indexed_scratch_bytes(i64(n_src), i64(n_dst), i64(nnz), i32(c_in), i32(c_out)),
            lib.sage_scatter_mean_det_scratch_bytes(i64(n_src), i64(n_dst), i64(nnz)),
            lib.sage_conv_forward_indexed_scratch_bytes(i64(n_dst), i32(c_in), i32(c_out))]


def table(lib):
    """[{args, off, on}]: the sizes with deterministic mode off and on."""
    rows = []
    was = lib.sage_set_deterministic(0)
    try:
        for args in cases.size_query_args():
            row = {"args": list(args)}
            for mode, key in ((0, "off"), (1, "on")):
                lib.sage_set_deterministic(mode)
                row[key] = sizes(lib, args)
            rows.append(row)
    finally:
        lib.sage_set_deterministic(was)
    return rows


if __name__ == "__main__":
    out = {"queries": list(QUERIES), "rows": table(ctypes.CDLL(os.path.abspath(sys.argv[1])))}
    print("{\n \"queries\": %s,\n \"rows\": [\n  %s\n ]\n}" % (json.dumps(out["queries"]), ",\n  ".join(json.dumps(r) for r in out["rows"])))
