"""Item-based CF on request from a prepared job, the parts that need no GPU: the ABI additions and the argument checks."""
import ctypes as C
import os
import re

from util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fy_itemcf_recommend_prepared", "fy_result_itemcf_request_stats", "fy_itemsim_job_drop_rows")


def test_header_symbols_and_library_agree():
    P = pkg()
    P.build()
    lib = P._native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "filmyou.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fy_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in P._native.SYMBOLS and hasattr(lib, name), name
    assert "fy_itemcf_request_stats;" in header
    assert lib.fy_abi_version() == 5      # purely additive


def test_struct_sizes():
    N = pkg()._native
    assert C.sizeof(N.ItemCFRequestStats) == 64
    assert [k for k, _ in N.ItemCFRequestStats._fields_] == ["users_asked", "users_known", "items_needed", "rows_built", "rows_from_store",
                                                              "rows_stored", "pair_contribs", "batches"]
    # no existing struct changed
    assert C.sizeof(N.Stats) == 33 * 8 and C.sizeof(N.ItemCFParams) == 24 and C.sizeof(N.ItemSimParams) == 48
    assert C.sizeof(N.ItemCFFilter) == 40 and C.sizeof(N.ItemSimRequestStats) == 48


def test_null_arguments_fail_cleanly():
    P = pkg()
    lib = P._native.load()
    p = P._native.ItemCFParams(10, 50, 0, 0, 1, 0)
    f = P._native.ItemCFFilter(1, 0, 0, None, 0, None)
    out = C.c_void_p(1)
    assert lib.fy_itemcf_recommend_prepared(None, C.byref(p), C.byref(f), C.byref(out)) == -1      # no job
    assert not out.value and b"NULL" in lib.fy_last_error()
    assert lib.fy_itemcf_recommend_prepared(None, C.byref(p), C.byref(f), None) == -1 and b"out" in lib.fy_last_error()
    assert lib.fy_itemcf_recommend_prepared(C.c_void_p(1), C.byref(p), C.byref(f), None) == -1      # (out is looked at before the job)
    st = P._native.ItemCFRequestStats()
    assert lib.fy_result_itemcf_request_stats(None, C.byref(st)) == -1 and b"NULL" in lib.fy_last_error()
    assert lib.fy_result_itemcf_request_stats(None, None) == -1
    lib.fy_itemsim_job_drop_rows(None)      # a no-op
