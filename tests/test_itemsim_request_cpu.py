"""Item similarity on request, the parts that need no GPU: the ABI additions, argument checks, the host layer's option handling."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fy_itemsim_prepare", "fy_itemsim_job_destroy", "fy_itemsim_rows", "fy_result_itemsim_request_stats")


def test_header_symbols_and_library_agree():
    P = pkg()
    P.build()
    lib = P._native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "filmyou.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fy_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in P._native.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"typedef struct \{ int64_t n_items; const int32_t\* items; \} fy_itemsim_request;", header)
    assert "typedef struct fy_itemsim_job fy_itemsim_job;" in header and "fy_itemsim_request_stats;" in header
    assert lib.fy_abi_version() == 5      # purely additive


def test_struct_sizes():
    N = pkg()._native
    assert C.sizeof(N.ItemSimRequest) == 16
    assert C.sizeof(N.ItemSimRequestStats) == 48
    assert C.sizeof(N.ItemSimParams) == 48 and C.sizeof(N.Stats) == 33 * 8


def test_null_arguments_fail_cleanly():
    P = pkg()
    lib = P._native.load()
    rq = P._native.ItemSimRequest(0, None)
    out = C.c_void_p(1)
    assert lib.fy_itemsim_rows(None, C.byref(rq), C.byref(out)) == -1
    assert not out.value and lib.fy_last_error()
    assert lib.fy_itemsim_rows(None, C.byref(rq), None) == -1 and lib.fy_last_error()
    out = C.c_void_p(1)
    assert lib.fy_itemsim_rows(C.c_void_p(1), None, C.byref(out)) == -1      # (the request is looked at before the job)
    assert not out.value and lib.fy_last_error()
    p = P._native.ItemSimParams(0, 10, 1, 0, 0.0, 0, 1, 0, 1, 0)
    job = C.c_void_p(1)
    assert lib.fy_itemsim_prepare(None, C.byref(p), None, C.byref(job)) == -1
    assert not job.value and b"NULL" in lib.fy_last_error()
    assert lib.fy_itemsim_prepare(None, C.byref(p), None, None) == -1 and lib.fy_last_error()
    st = P._native.ItemSimRequestStats()
    assert lib.fy_result_itemsim_request_stats(None, C.byref(st)) == -1 and b"NULL" in lib.fy_last_error()
    assert lib.fy_result_itemsim_request_stats(None, None) == -1
    lib.fy_itemsim_job_destroy(None)      # a no-op


def test_items_file_is_read_before_any_device_work(tmp_path):
    """RowSimilarityJob.run(itemsFile=path) reads the file (read_id_file) before it prepares anything: a missing file fails without a
    device, a good one gets as far as the context."""
    P = pkg()

    class NoContext:      # any use of the context would fail
        def __getattr__(self, name):
            raise AssertionError("the device was touched")

    f = tmp_path / "items.txt"
    f.write_text("7\n\n  12  \nabc\n7\n12x\n99999999999\n-3\n5")
    assert P.read_id_file(str(f)).tolist() == [7, 12, 7, -3, 5]
    job = P.RowSimilarityJob(NoContext())
    with pytest.raises(P.FilmYouError):
        job.run(([1], [1], [1.0]), itemsFile=str(tmp_path / "missing.txt"))
    with pytest.raises(AssertionError, match="the device was touched"):
        job.run(([1], [1], [1.0]), itemsFile=str(f))
    with pytest.raises(AssertionError, match="the device was touched"):
        job.run(([1], [1], [1.0]), itemsFile=np.array([1, 2], dtype=np.int32))
