"""Named pairs explained by their contributing preferences: the statement (tests/because_ref.py) on a hand-written example with the
expected rows written out, the preconditions of the crafted "block" data from the measures' statement, the layouts of the two new
ABI structs and the NULL refusals.  No GPU."""
import ctypes as C
import math

import numpy as np

import because_ref as BR
import estimate_ref as ER
import itemsim_measures_ref as MR
from util import pkg

NAN = float("nan")
# 4 users x 6 items.  Raters per item: 3, 2, 1, 1, 1, 1 -- so the order of a user's preferences is the order of the item ids.
U = np.array([1, 1, 1, 1, 2, 2, 3, 3, 4], dtype=np.int32)
I = np.array([1, 2, 3, 4, 1, 2, 1, 5, 6], dtype=np.int32)
S = np.array([4.0, 2.0, 4.0, 1.0, 5.0, 3.0, 2.0, 2.0, 3.0], dtype=np.float32)
SIM = [(1, 5, 0.5), (1, 6, 0.25), (1, 2, 0.5),
       (2, 5, 1.0), (2, 6, NAN), (2, 1, 0.5),
       (3, 5, 0.5), (3, 6, 0.75),
       (4, 5, -2.0), (4, 6, 0.5),
       (5, 1, 0.5),
       (6, 1, 0.25)]
PAIRS = [(1, 5), (1, 6), (2, 5), (2, 6), (4, 1), (1, 1), (9, 1), (1, 99), (1, 5)]


def f32(x):
    return int(np.float32(x).view(np.uint32))


def hand(how_many, max_prefs=50, boolean=False):
    si, so, sv = (np.array(c) for c in zip(*SIM))
    pu, pi = (np.array(c, dtype=np.int32) for c in zip(*PAIRS))
    return BR.listed(BR.contributors(U, I, S, si, so, sv.astype(np.float32), pu, pi, max_prefs, boolean), how_many)


def test_hand_written_example():
    rows, cnt, start = hand(3)
    assert cnt.tolist() == [4, 4, 2, 2, 1, 1, 0, 0, 4]
    assert start.tolist() == [0, 3, 6, 8, 10, 11, 12, 12, 12, 15]
    assert rows == [
        # (1, 5): weights 4 * 0.5 = 2 * 1.0 = 4 * 0.5 = 2.0 -- a three-way tie by ascending id -- and 1 * -2.0 behind them, cut off
        (0, 1, f32(0.5), f32(4.0)), (0, 2, f32(1.0), f32(2.0)), (0, 3, f32(0.5), f32(4.0)),
        # (1, 6): 3.0, 1.0, 0.5 and the NaN of item 2 last, cut off
        (1, 3, f32(0.75), f32(4.0)), (1, 1, f32(0.25), f32(4.0)), (1, 4, f32(0.5), f32(1.0)),
        # (2, 5): 3 * 1.0 before 5 * 0.5
        (2, 2, f32(1.0), f32(3.0)), (2, 1, f32(0.5), f32(5.0)),
        # (2, 6): the number before the NaN
        (3, 1, f32(0.25), f32(5.0)), (3, 2, f32(NAN), f32(3.0)),
        # (4, 1): one contributor (the estimate is TOO_FEW; the term is listed all the same)
        (4, 6, f32(0.25), f32(3.0)),
        # (1, 1): the user's own preference; the row of item 2 holds item 1
        (5, 2, f32(0.5), f32(2.0)),
        # (9, 1), (1, 99): unknown user, unknown item: nothing; then (1, 5) again
        (8, 1, f32(0.5), f32(4.0)), (8, 2, f32(1.0), f32(2.0)), (8, 3, f32(0.5), f32(4.0))]
    # all four of (1, 5) and (1, 6): the negative weight and the NaN come last
    rows, cnt, start = hand(64)
    assert [r[1] for r in rows[start[0]:start[1]]] == [1, 2, 3, 4] and [r[1] for r in rows[start[1]:start[2]]] == [3, 1, 4, 2]
    assert math.isnan(np.uint32(rows[start[1] + 3][2]).view(np.float32))
    rows, cnt, start = hand(1)
    assert [r[:2] for r in rows] == [(0, 1), (1, 3), (2, 2), (3, 1), (4, 6), (5, 2), (8, 1)] and cnt.tolist() == [4, 4, 2, 2, 1, 1, 0, 0, 4]
    # boolean data: pref 1, weight = sim: 1.0, then 0.5 twice by id, then -2.0
    rows, cnt, start = hand(64, boolean=True)
    assert [r[1] for r in rows[start[0]:start[1]]] == [2, 1, 3, 4] and {r[3] for r in rows} == {f32(1.0)}
    # maxPrefs 2: user 1 keeps the two 4.0 (items 1 and 3)
    rows, cnt, start = hand(64, max_prefs=2)
    assert [r[1] for r in rows[start[0]:start[1]]] == [1, 3] and cnt.tolist()[:2] == [2, 2]


def test_the_terms_fold_to_the_statements_estimate():
    si, so, sv = (np.array(c) for c in zip(*SIM))
    pu, pi = (np.array(c, dtype=np.int32) for c in zip(*PAIRS))
    value, status = ER.estimate(U, I, S, si, so, sv, pu, pi, 50)
    allc = BR.contributors(U, I, S, si, so, sv, pu, pi, 50)
    assert status.tolist() == [ER.OK, ER.NOT_A_NUMBER, ER.OK, ER.NOT_A_NUMBER, ER.TOO_FEW, ER.OWN_PREFERENCE, ER.UNKNOWN_USER, ER.UNKNOWN_ITEM, ER.OK]
    for t in np.flatnonzero(status == ER.OK):
        assert BR.fold([(v, p) for _, v, p, _ in allc[t]]) == np.float32(value[t])
    assert value[0] == (2.0 + 2.0 + 2.0 - 2.0) / (0.5 + 1.0 + 0.5 + 2.0)


def test_block_preconditions_from_the_measures_statement():
    u, i, s = BR.block_data()
    assert len(u) == BR.BLOCK_USERS * BR.BLOCK_ITEMS - 5 and (s[u == BR.BLOCK_X] == 4.0).all() and (u == BR.BLOCK_X).sum() == 75
    a, b = BR.BLOCK_TWINS
    assert a < b and np.array_equal(s[i == a], s[i == b]) and np.array_equal(u[i == a], u[i == b])
    ref = MR.itemsim(u, i, s, MR.COSINE, max_similarities_per_item=100)
    assert len(ref["item"]) == 80 * 79                                    # every row holds every other item
    pu = np.full(5, BR.BLOCK_X, dtype=np.int32)
    pi = np.array(BR.BLOCK_LACKS, dtype=np.int32)
    sims32 = ref["sim"].astype(np.float32)
    allc = BR.contributors(u, i, s, ref["item"], ref["other"], sims32, pu, pi, 10)
    assert [len(c) for c in allc] == [75] * 5                             # ties at the cut keep all 75 preferences
    for c in allc:
        best = sorted(c, key=BR.order_key)
        k = [e[0] for e in best].index(a)
        assert best[k + 1][0] == b and best[k][3] == best[k + 1][3]       # equal weights, ascending ids
    rows, cnt, start = BR.listed(allc, 64)
    assert cnt.tolist() == [75] * 5 and np.diff(start).tolist() == [64] * 5


def test_struct_sizes_and_abi_version():
    P = pkg()
    P.build()
    N = P._native
    assert N.FY_BECAUSE_MAX == 64
    assert C.sizeof(N.ItemCFBecauseView) == 64 and N.ItemCFBecauseView.start.offset == 8 and N.ItemCFBecauseView.pref.offset == 56
    assert N.ItemCFBecauseView.estimate.offset == 32 and N.ItemCFBecauseView.contributors.offset == 48
    assert C.sizeof(N.ItemCFBecauseStats) == 168 and N.ItemCFBecauseStats.row_entries_walked.offset == 160
    assert N.ItemCFBecauseStats.by_status.offset == 16 and N.ItemCFBecauseStats.users_known.offset == 80
    assert N.ItemCFBecauseStats.rows.offset == 96 and N.ItemCFBecauseStats.contributors.offset == 104 and N.ItemCFBecauseStats.items_needed.offset == 112
    assert N.load().fy_abi_version() == 5


def test_null_arguments_without_a_device():
    P = pkg()
    N = P._native
    lib = N.load()
    out = C.c_void_p(1)
    prm, pairs = N.ItemCFParams(0, 50, 0, 0, 1, 0), N.ItemCFPairs(0, None, None, 0)
    assert lib.fy_itemcf_because_prepared(None, C.byref(prm), C.byref(pairs), 5, C.byref(out)) == -1 and not out.value
    assert b"NULL" in lib.fy_last_error()
    assert lib.fy_itemcf_because_prepared(None, C.byref(prm), C.byref(pairs), 5, None) == -1
    assert lib.fy_result_because_view(None, C.byref(N.ItemCFBecauseView())) == -1
    assert lib.fy_result_itemcf_because_stats(None, C.byref(N.ItemCFBecauseStats())) == -1
