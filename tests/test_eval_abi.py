"""CPU-side checks of the evaluation-metrics export (include/graphpope_hip.h: sage_eval_metrics; main.py:216-217, 227-228, 238):
it loads, the header declares it, and bad arguments are refused before any HIP call."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_metrics_is_exported_and_declared():
    from graphpope_amd import _lib
    lib = _lib.load()
    assert "sage_eval_metrics" in _lib.SIGNATURES and hasattr(lib, "sage_eval_metrics")
    with open(os.path.join(ROOT, "include", "graphpope_hip.h")) as f:
        header = f.read()
    decl = re.search(r"\bint\s+sage_eval_metrics\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/graphpope_hip.h does not declare sage_eval_metrics"
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["sage_eval_metrics"][1]) == 8
    assert "main.py:216-217" in header and "227-228, 238" in header         # the comment cites what the entry point replaces


@pytest.mark.parametrize("case", ["logits", "target", "acc", "bad_label", "M=0", "M=2^31", "C=0"])
def test_eval_metrics_validates_before_any_hip_call(case):
    """sage_eval_metrics(logits, target, M, C, ignore_index, acc, bad_label, stream): ERR_INVALID with its name in the message."""
    from graphpope_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(64)                     # a non-null address that is never dereferenced: every call below fails validation first
    ptrs = {"logits": one, "target": one, "acc": one, "bad_label": one}
    m, c = 5, 3
    if case in ptrs:
        ptrs[case] = null
    elif case == "M=0":
        m = 0
    elif case == "M=2^31":
        m = 2 ** 31
    else:
        c = 0
    code = lib.sage_eval_metrics(ptrs["logits"], ptrs["target"], m, c, -100, ptrs["acc"], ptrs["bad_label"], null)
    assert code == _lib.ERR_INVALID, case
    msg = lib.pope_last_error()
    assert b"sage_eval_metrics" in msg, (case, msg)
    assert (b"null pointer" in msg) == (case in ("logits", "target", "acc", "bad_label")), (case, msg)
    assert lib.pope_n2v_windows(null, 0, 8, 4, null, null) == _lib.OK and lib.pope_last_error() == b""     # an empty call: leaves no message behind
