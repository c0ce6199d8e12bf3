"""Ratings that take writes, host side: the plain statement of the contract (tests/ratings_update_ref.py) on hand-written cases, one
per rule; the ctypes layout of fy_ratings_update_stats against the header; argument validation of fy_ratings_apply.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

from ratings_update_ref import COUNTERS, apply_writes, same_bits
from util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = ([1, 1, 2, 3], [10, 11, 10, 12], [4.0, 3.0, 5.0, 2.5])          # (user, item, score), in this order


def rows(out):
    return list(zip(out[0].tolist(), out[1].tolist(), out[2].tolist()))


def counters(c, **want):
    full = dict.fromkeys(COUNTERS, 0)
    full.update(want)
    return c == full


def test_rule1_the_last_write_per_key_counts():
    out = apply_writes(*SRC, [1, 1, 1], [10, 10, 10], [1.0, 2.0, 0.5])
    assert rows(out) == [(1, 11, 3.0), (2, 10, 5.0), (3, 12, 2.5), (1, 10, 0.5)]
    assert counters(out[3], n_writes=3, n_superseded=2, n_replaced=1, n_source_dropped=1, nnz_out=4)
    # write / delete / write of one key: the row is there, with the last score, at the place of the LAST write
    out = apply_writes(*SRC, [2, 9, 2, 2], [10, 9, 10, 10], [1.0, 7.0, 0.0, 3.5], [0, 0, 1, 0])
    assert rows(out) == [(1, 10, 4.0), (1, 11, 3.0), (3, 12, 2.5), (9, 9, 7.0), (2, 10, 3.5)]
    assert counters(out[3], n_writes=4, n_superseded=2, n_replaced=1, n_inserted=1, n_source_dropped=1, nnz_out=5)
    # write / delete of one key: gone, for a key of the source and for a new one
    out = apply_writes(*SRC, [2, 2, 8, 8], [10, 10, 8, 8], [1.0, 9.0, 1.0, 9.0], [0, 1, 0, 1])
    assert rows(out) == [(1, 10, 4.0), (1, 11, 3.0), (3, 12, 2.5)]
    assert counters(out[3], n_writes=4, n_superseded=2, n_deleted=1, n_delete_missed=1, n_source_dropped=1, nnz_out=3)


def test_rule2_every_source_entry_of_a_named_key_is_dropped():
    dup = ([1, 2, 1, 3, 1], [10, 10, 10, 12, 10], [4.0, 5.0, 1.0, 2.5, 2.0])      # (1, 10) three times
    out = apply_writes(*dup, [1], [10], [3.0])                                    # a write cures the duplicate
    assert rows(out) == [(2, 10, 5.0), (3, 12, 2.5), (1, 10, 3.0)]
    assert counters(out[3], n_writes=1, n_replaced=1, n_source_dropped=3, nnz_out=3)
    out = apply_writes(*dup, [1], [10], [3.0], [1])                               # ... and so does a delete
    assert rows(out) == [(2, 10, 5.0), (3, 12, 2.5)]
    assert counters(out[3], n_writes=1, n_deleted=1, n_source_dropped=3, nnz_out=2)
    out = apply_writes(*dup, [3], [12], [1.5])                                    # a duplicate the batch does not touch stays
    assert rows(out) == [(1, 10, 4.0), (2, 10, 5.0), (1, 10, 1.0), (1, 10, 2.0), (3, 12, 1.5)]
    assert counters(out[3], n_writes=1, n_replaced=1, n_source_dropped=1, nnz_out=5)


def test_rule3_source_order_then_batch_order():
    out = apply_writes(*SRC, [7, 3, 5, 1], [1, 12, 1, 11], [1.0, 2.0, 3.0, 4.0])
    assert rows(out) == [(1, 10, 4.0), (2, 10, 5.0), (7, 1, 1.0), (3, 12, 2.0), (5, 1, 3.0), (1, 11, 4.0)]
    assert counters(out[3], n_writes=4, n_replaced=2, n_inserted=2, n_source_dropped=2, nnz_out=6)


def test_rule4_scores_are_data():
    nan = np.float32(np.nan)
    out = apply_writes(*SRC, [1, 2, -5, 4], [10, 10, -6, 4], [0.0, -2.0, 1.0, nan])
    assert rows(out)[:5] == [(1, 11, 3.0), (3, 12, 2.5), (1, 10, 0.0), (2, 10, -2.0), (-5, -6, 1.0)]
    assert out[0][5] == 4 and np.isnan(out[2][5]) and out[2].dtype == np.float32
    assert counters(out[3], n_writes=4, n_replaced=2, n_inserted=2, n_source_dropped=2, nnz_out=6)
    assert same_bits(np.float32([-0.0]), apply_writes([], [], [], [1], [1], [-0.0])[2])
    assert not same_bits(np.float32([0.0]), np.float32([-0.0]))


def test_rule5_and_6_empty_batch_empty_source():
    out = apply_writes(*SRC, [], [], [])
    assert rows(out) == list(zip(*SRC)) and counters(out[3], nnz_out=4)
    out = apply_writes([], [], [], [5, 5, 6, 7], [1, 1, 1, 1], [1.0, 2.0, 3.0, 4.0], [0, 0, 0, 1])
    assert rows(out) == [(5, 1, 2.0), (6, 1, 3.0)]
    assert counters(out[3], n_writes=4, n_superseded=1, n_inserted=2, n_delete_missed=1, nnz_out=2)
    big = 2 ** 31 - 1
    out = apply_writes([0, big], [big, 0], [1.0, 2.0], [big, 0], [0, big], [3.0, 4.0])
    assert rows(out) == [(big, 0, 3.0), (0, big, 4.0)] and out[0].max() == big == out[1].max()


def test_stats_struct_matches_the_header():
    P = pkg()
    header = open(os.path.join(ROOT, "include", "filmyou.h")).read()
    m = re.search(r"typedef struct \{ int64_t ([a-z_,\s]+); \} fy_ratings_update_stats;", header)
    assert m, "fy_ratings_update_stats is not declared as eight int64_t"
    names = [x.strip() for x in m.group(1).split(",")]
    S = P._native.RatingsUpdateStats
    assert names == [f for f, _ in S._fields_] == list(COUNTERS)
    assert all(t is C.c_int64 for _, t in S._fields_) and C.sizeof(S) == 64
    assert [getattr(S, f).offset for f in names] == list(range(0, 64, 8))
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(fy_[a-z0-9_]+)\s*\(", bare))
    P.build()
    lib = P._native.load()
    for name in ("fy_ratings_apply", "fy_ratings_copy_out"):
        assert name in declared and name in P._native.SYMBOLS and hasattr(lib, name), name
    assert lib.fy_abi_version() == 5      # purely additive
    assert hasattr(P.Ratings, "updated") and hasattr(P.Ratings, "to_host")


def test_argument_validation_without_a_device():
    P = pkg()
    P.build()
    lib = P._native.load()
    a = np.array([1, 2, 3], dtype=np.int32)
    s = np.array([1, 2, 3], dtype=np.float32)
    pa, ps = a.ctypes.data, s.ctypes.data

    def call(ctx, src, n, u, i, sc, loc, out):
        return lib.fy_ratings_apply(ctx, src, n, u, i, sc, None, loc, out, None)

    out = C.c_void_p(1)
    assert call(None, None, 3, pa, pa, ps, 0, C.byref(out)) == -1                   # NULL context (and source)
    assert out.value is None and b"NULL" in lib.fy_last_error()
    assert call(None, None, 3, pa, pa, ps, 0, None) == -1                           # NULL out
    assert b"out" in lib.fy_last_error()
    out = C.c_void_p(1)
    assert call(None, None, -1, pa, pa, ps, 0, C.byref(out)) == -1 and out.value is None
    assert b"n < 0" in lib.fy_last_error()
    for u, i, sc in ((None, pa, ps), (pa, None, ps), (pa, pa, None)):               # NULL arrays with n > 0
        out = C.c_void_p(1)
        assert call(None, None, 3, u, i, sc, 0, C.byref(out)) == -1 and out.value is None
        assert b"arrays are NULL" in lib.fy_last_error()
    out = C.c_void_p(1)
    assert call(None, None, 3, pa, pa, ps, 2, C.byref(out)) == -1 and out.value is None
    assert b"location" in lib.fy_last_error()
    assert lib.fy_ratings_copy_out(None, pa, pa, ps) == -1
