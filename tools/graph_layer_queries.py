"""Every host-side answer of the whole-graph layers (GCNConv, GATConv, GATv2Conv, full-graph SAGE inference) and of the SAGE backward name
query over a fixed grid, one line each, from a library given by path:
    python tools/graph_layer_queries.py path/to/libgraphpope_hip.so | sha256sum
The kernel-name queries, the scratch-size queries, and the refusals of the entry points (return code and pope_last_error) that happen
before any HIP call.  Two builds whose host code says the same print the same bytes: run it on a build of the commit whose answers are to
be kept and on the tree under test, and compare.  Host logic: needs no GPU."""
import itertools
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gatv2_cases  # noqa: E402
import gcn_cases  # noqa: E402
from graphpope_amd import _lib  # noqa: E402

NS = (1, 17, 300, 89250)
NNZS = (0, 512, 513, 5000, 899756)          # hubs = nnz > 512
C_INS = (12, 36, 500)
GCN_C_OUTS = tuple(co for _, co in gcn_cases.SHAPES + (gcn_cases.WHOLE_TILE_SHAPE,))
HEADS = tuple((h, c) for _, h, c in gatv2_cases.SHAPES) + ((8, 32), (1, 7))
CUS = (256, 64)
BOTH = (0, 1)
CAP = 2048


def masks(bits):
    return (0,) + tuple(1 << b for b in range(bits)) + ((1 << bits) - 1,)


def name_line(lib, buf, query, args):
    rc = getattr(lib, query)(*args, buf, CAP)
    return "%s%r -> %s" % (query, args, buf.value.decode() if rc == 0 else "rc %d: %s" % (rc, lib.pope_last_error().decode()))


def name_lines(lib):
    buf = _lib.ctypes.create_string_buffer(CAP)
    for n, nnz, c_in, cus in itertools.product(NS, NNZS, C_INS, CUS):
        for c_out, backward, grad_x, mask in itertools.product(GCN_C_OUTS, BOTH, BOTH, masks(5)):
            yield name_line(lib, buf, "pope_gcn_kernel_name", (n, nnz, c_in, c_out, backward, grad_x, cus, mask))
        for c_out, has_bn, mask in itertools.product(GCN_C_OUTS, BOTH, masks(3)):
            yield name_line(lib, buf, "sage_full_layer_kernel_name", (n, nnz, c_in, c_out, has_bn, cus, mask))
        for (h, c), concat, backward, grad_x in itertools.product(HEADS, BOTH, BOTH, BOTH):
            for mask in masks(6):
                yield name_line(lib, buf, "pope_gat_kernel_name", (n, nnz, c_in, h, c, concat, backward, grad_x, cus, mask))
            for share, mask in itertools.product(BOTH, masks(9)):
                yield name_line(lib, buf, "pope_gatv2_kernel_name", (n, nnz, c_in, h, c, concat, share, backward, grad_x, cus, mask))
    was = lib.sage_set_deterministic(0)
    try:
        for det in BOTH:
            lib.sage_set_deterministic(det)
            for n_dst, c_in, cus, c_out, grad_x, grad_b, mask in itertools.product(NS, C_INS, CUS, GCN_C_OUTS, BOTH, BOTH, masks(9)):
                for n_src in (n_dst, 2 * n_dst + 1):              # (the index bit with need_grad_x: a refusal, printed as one)
                    yield "det=%d " % det + name_line(lib, buf, "sage_backward_kernel_name_at", (n_dst, n_src, c_in, c_out, grad_x, grad_b, cus, mask))
    finally:
        lib.sage_set_deterministic(was)


def size_lines(lib):
    def line(query, args):
        return "%s%r -> %d" % (query, args, getattr(lib, query)(*args))
    for n, nnz in itertools.product(NS + (0,), NNZS + (-1,)):
        for c in GCN_C_OUTS + (0,):
            yield line("pope_gcn_propagate_scratch_size", (n, nnz, c))
        for c_in, c_out in itertools.product(C_INS + (0,), GCN_C_OUTS):
            for query in ("pope_gcn_conv_forward_scratch_size", "pope_gcn_conv_backward_scratch_size", "sage_full_layer_scratch_size"):
                yield line(query, (n, nnz, c_in, c_out))
        for (h, c), concat in itertools.product(HEADS + ((0, 4),), BOTH):
            yield line("pope_gat_propagate_scratch_size", (n, nnz, h, c, concat))
            for c_in in C_INS:
                for query in ("pope_gat_conv_forward_scratch_size", "pope_gat_conv_backward_scratch_size", "pope_gatv2_conv_forward_scratch_size",
                              "pope_gatv2_conv_backward_scratch_size"):
                    yield line(query, (n, nnz, c_in, h, c, concat))


# ---- the refusals of the entry points ----
# Every call below is refused by the argument checks, before the first HIP call, so no pointer is followed: only a REQUIRED pointer is
# nulled, only a size that must be positive is zeroed, only the aliases the contract forbids are tried.  (A variation the library accepts
# would launch kernels on made-up addresses: never add one.)
VALUES = {"N": 10, "nnz": 20, "c_in": 4, "c_out": 8, "C8": 8, "H": 2, "C": 4, "concat": 1, "mean": 0, "self_w": 1.0, "slope": 0.2, "loops": 1, "eps": 1e-5,
          "stream": None}
GRAPH = "rowptr col N nnz"
BOTH_CSR = "rowptr col rowptr_t col_t slot_map N nnz"
ENTRIES = (   # (entry point, parameters in order, its scratch query and that query's arguments, the refusing variations)
    ("pope_gcn_propagate", GRAPH + " dinv self_w h C8 bias out scratch bytes stream", ("pope_gcn_propagate_scratch_size", "N nnz C8"),
     "null:rowptr,col,h,out,scratch zero:N,C8 huge:N,nnz set:self_w=-1,self_w=1e7,self_w=nan alias:out=h"),
    ("pope_gcn_conv_forward", GRAPH + " dinv self_w x c_in weight bias c_out out scratch bytes stream",
     ("pope_gcn_conv_forward_scratch_size", "N nnz c_in c_out"), "null:rowptr,col,x,weight,out,scratch zero:N,c_in,c_out huge:N,nnz set:self_w=-1,self_w=nan"),
    ("pope_gcn_conv_backward", GRAPH + " dinv self_w x c_in weight c_out grad_out grad_x grad_weight grad_bias scratch bytes stream",
     ("pope_gcn_conv_backward_scratch_size", "N nnz c_in c_out"),
     "null:rowptr,col,x,weight,grad_out,grad_weight,scratch zero:N,c_in,c_out huge:N,nnz set:self_w=-1,self_w=nan"),
    ("pope_gat_attention", GRAPH + " h H C att_l att_r slope loops a_src a_dst alpha alpha_self stream", None,
     "null:rowptr,col,h,att_l,att_r,a_src,a_dst,alpha,alpha_self zero:N,H,C huge:N,nnz,H set:slope=2,slope=-0.5,slope=nan"),
    ("pope_gat_propagate", GRAPH + " alpha alpha_self h H C mean bias out scratch bytes stream", ("pope_gat_propagate_scratch_size", "N nnz H C mean"),
     "null:rowptr,col,alpha,h,out,scratch zero:N,H,C huge:N,nnz,H alias:out=h"),
    ("pope_gat_conv_forward", GRAPH + " x c_in weight att_l att_r bias H C concat slope loops h a_src a_dst alpha alpha_self out scratch bytes stream",
     ("pope_gat_conv_forward_scratch_size", "N nnz c_in H C concat"),
     "null:rowptr,col,x,weight,att_l,att_r,h,a_src,a_dst,alpha,alpha_self,out,scratch zero:N,c_in,H,C huge:N,nnz,H set:slope=2,slope=nan"),
    ("pope_gat_conv_backward", BOTH_CSR + " x c_in weight att_l att_r H C concat slope loops h a_src a_dst alpha alpha_self grad_out grad_x grad_weight"
     " grad_att_l grad_att_r grad_bias scratch bytes stream", ("pope_gat_conv_backward_scratch_size", "N nnz c_in H C concat"),
     "null:rowptr,col,rowptr_t,col_t,slot_map,x,weight,att_l,att_r,h,a_src,a_dst,alpha,alpha_self,grad_out,grad_weight,grad_att_l,grad_att_r,scratch"
     " zero:N,c_in,H,C huge:N,nnz,H set:slope=2,slope=nan"),
    ("pope_gatv2_scores", GRAPH + " hl hr H C att slope loops e e_self stream", None,
     "null:rowptr,col,hl,hr,att,e,e_self zero:N,H,C huge:N,nnz,H set:slope=2,slope=nan"),
    ("pope_gatv2_attention", GRAPH + " hl hr H C att slope loops e e_self alpha alpha_self stream", None,
     "null:rowptr,col,hl,hr,att,e,e_self,alpha,alpha_self zero:N,H,C huge:N,nnz,H set:slope=2,slope=nan"),
    ("pope_gatv2_conv_forward", GRAPH + " x c_in weight_l bias_l weight_r bias_r att bias H C concat slope loops hl hr alpha alpha_self out scratch bytes stream",
     ("pope_gatv2_conv_forward_scratch_size", "N nnz c_in H C concat"),
     "null:rowptr,col,x,weight_l,att,hl,hr,alpha,alpha_self,out,scratch zero:N,c_in,H,C huge:N,nnz,H set:slope=2,slope=nan"
     " alias:hr=hl,out=hl,out=hr,out=alpha,out=alpha_self"),
    ("pope_gatv2_conv_backward", BOTH_CSR + " x c_in weight_l weight_r att H C concat slope loops hl hr alpha alpha_self grad_out grad_x grad_weight_l"
     " grad_bias_l grad_weight_r grad_bias_r grad_att grad_bias scratch bytes stream", ("pope_gatv2_conv_backward_scratch_size", "N nnz c_in H C concat"),
     "null:rowptr,col,rowptr_t,col_t,slot_map,x,weight_l,att,hl,hr,alpha,alpha_self,grad_out,grad_weight_l,grad_weight_r,grad_att,scratch"
     " zero:N,c_in,H,C huge:N,nnz,H set:slope=2,slope=nan"),
    ("sage_full_layer_forward", GRAPH + " x c_in w_l b_l w_r c_out gamma beta mean_ var eps out scratch bytes stream",
     ("sage_full_layer_scratch_size", "N nnz c_in c_out"), "null:rowptr,col,x,w_l,w_r,out,scratch,gamma,beta,mean_,var zero:N,c_in,c_out huge:N,nnz,c_out"),
)


def refusal_lines(lib):
    for name, params, query, variations in ENTRIES:
        params = params.split()
        need = getattr(lib, query[0])(*(VALUES[k] for k in query[1].split())) if query else 0
        base = {k: VALUES[k] if k in VALUES else need if k == "bytes" else 4096 * (i + 1) for i, k in enumerate(params)}
        cases = []
        for group in variations.split():
            kind, items = group.split(":")
            for item in items.split(","):
                if kind == "null":
                    cases.append(("%s = NULL" % item, {item: None}))
                elif kind == "zero":
                    cases.append(("%s = 0" % item, {item: 0}))
                elif kind == "huge":
                    cases.append(("%s = INT32_MAX" % item, {item: 2 ** 31 - 1}))
                else:
                    k, v = item.split("=")
                    cases.append((item, {k: float(v) if kind == "set" else base[v]}))
        if query:
            cases += [("one byte short", {"bytes": need - 1}), ("no bytes", {"bytes": 0})]
        for what, over in cases:
            rc = getattr(lib, name)(*({**base, **over}[k] for k in params))
            if rc == 0 or b"failed:" in lib.pope_last_error():           # it went on to a HIP call: the variation is no refusal, take it out
                raise SystemExit("%s [%s] was accepted" % (name, what))
            yield "%s [%s] -> rc %d: %s" % (name, what, rc, lib.pope_last_error().decode())
    buf = _lib.ctypes.create_string_buffer(CAP)
    for query, args in (("pope_gcn_kernel_name", (300, 10, 36, 256, 0, 1, 256, 0)), ("pope_gat_kernel_name", (300, 5000, 36, 4, 64, 1, 1, 1, 256, 0)),
                        ("pope_gatv2_kernel_name", (300, 5000, 36, 4, 64, 1, 0, 1, 1, 256, 0)), ("sage_full_layer_kernel_name", (300, 10, 36, 256, 0, 256, 0)),
                        ("sage_backward_kernel_name_at", (300, 600, 36, 256, 1, 1, 256, 0))):
        for cap in (1, 8, 16, 64):
            rc = getattr(lib, query)(*args, buf, cap)
            yield "%s%r cap %d -> rc %d: %s" % (query, args, cap, rc, lib.pope_last_error().decode())
        yield "%s%r no buffer -> rc %d: %s" % (query, args, getattr(lib, query)(*args, None, CAP), lib.pope_last_error().decode())
        for i in range(len(args)):
            for v in (0, -1):
                bad = args[:i] + (v,) + args[i + 1:]
                if bad != args and not (v == -1 and i == len(args) - 1):          # (the mask is unsigned)
                    yield name_line(lib, buf, query, bad)


if __name__ == "__main__":
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    lib = _lib.load()
    for lines in (name_lines(lib), size_lines(lib), refusal_lines(lib)):
        for text in lines:
            print(text)
