"""RM2 on request, the parts that need no GPU: the ABI additions, argument checks, the host layer's option handling."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fy_rm2_score_users", "fy_result_request_stats")


def test_header_symbols_and_library_agree():
    P = pkg()
    P.build()
    lib = P._native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "filmyou.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fy_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in P._native.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"typedef struct \{ int64_t n_users; const int32_t\* users; \} fy_rm2_request;", header)
    assert "fy_rm2_request_stats;" in header
    assert lib.fy_abi_version() == 5      # purely additive


def test_struct_sizes():
    P = pkg()
    assert C.sizeof(P._native.RM2Request) == 16
    assert C.sizeof(P._native.RM2RequestStats) == 64
    assert C.sizeof(P._native.RM2Params) == 48 and C.sizeof(P._native.Stats) == 33 * 8


def test_null_arguments_fail_cleanly():
    P = pkg()
    lib = P._native.load()
    out = C.c_void_p(1)
    rq = P._native.RM2Request(0, None)
    assert lib.fy_rm2_score_users(None, C.byref(rq), C.byref(out)) == -1
    assert not out.value and lib.fy_last_error()
    assert lib.fy_rm2_score_users(None, C.byref(rq), None) == -1
    st = P._native.RM2RequestStats()
    assert lib.fy_result_request_stats(None, C.byref(st)) == -1 and b"NULL" in lib.fy_last_error()
    assert lib.fy_result_request_stats(None, None) == -1


def test_users_file_with_collectives_is_refused_before_any_device_work():
    P = pkg()
    conf = P.Configuration()
    conf.setInt("numberOfItems", 5)
    conf.setInt("numberOfClusters", 1)

    class NoContext:      # any use of the context would fail
        def __getattr__(self, name):
            raise AssertionError("the device was touched")

    job = P.RM2Job(conf, NoContext())
    with pytest.raises(ValueError, match="usersFile"):
        job.run(([1], [1], [1.0]), usersFile=[1], collectives=object())


def test_users_file_is_read_before_any_device_work(tmp_path):
    """RM2Job.run(usersFile=path) reads the file as read_id_file documents (blank lines, non-integers and ids outside int32 skipped,
    duplicates kept) before it prepares anything: a missing file fails without a device, a good one gets as far as the context."""
    P = pkg()
    conf = P.Configuration()
    conf.setInt("numberOfItems", 5)
    conf.setInt("numberOfClusters", 1)

    class NoContext:
        def __getattr__(self, name):
            raise AssertionError("the device was touched")

    f = tmp_path / "users.txt"
    f.write_text("7\n\n  12  \nabc\n7\n12x\n99999999999\n-3\n5")
    ids = P.read_id_file(str(f))
    assert ids.dtype == np.int32 and ids.tolist() == [7, 12, 7, -3, 5]
    job = P.RM2Job(conf, NoContext())
    with pytest.raises(P.FilmYouError):
        job.run(([1], [1], [1.0]), usersFile=str(tmp_path / "missing.txt"))
    with pytest.raises(AssertionError, match="the device was touched"):
        job.run(([1], [1], [1.0]), usersFile=str(f))
