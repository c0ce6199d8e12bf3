"""The statement of the offline evaluation (tests/eval_ref.py) pinned by hand, the layouts of the new ABI structs, and the hold-out
hash on the reference's own RM2 fixture.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import eval_ref
from util import pkg


def one_list(items, R, N, gain="binary", threshold=1.0):
    test = (np.full(len(R), 7, dtype=np.int32), np.array(list(R), dtype=np.int32), np.array([R[i] for i in R], dtype=np.float32))
    e = eval_ref.evaluate(np.full(len(items), 7, dtype=np.int32), np.array(items, dtype=np.int32), test, (N,), threshold, gain)
    return e, {k: e["per_user"][k][0, 0] for k in eval_ref.VALUES}


def test_the_hand_computed_list():
    e, v = one_list([10, 20, 30, 40], {20: 5.0, 40: 5.0, 99: 5.0}, 4)
    assert v["hits"] == 2 and e["hits"] == [2] and e["users_hit"] == [1]
    assert e["hits"][0] / 4 == 0.5                                    # precision divides by N
    assert v["recall"] == pytest.approx(2 / 3, rel=1e-15)
    assert v["ap"] == pytest.approx((1 / 2 + 2 / 4) / 3, rel=1e-15) and v["ap"] == pytest.approx(1 / 3, rel=1e-15)
    assert v["rr"] == 0.5
    want = (1 / math.log2(3) + 1 / math.log2(5)) / (1 + 1 / math.log2(3) + 1 / math.log2(4))
    assert v["ndcg"] == pytest.approx(want, rel=1e-15) and want == pytest.approx(0.49818925746641285, rel=1e-15)
    assert (e["lists"], e["users_evaluated"], e["lists_without_relevant"], e["relevant_users"], e["relevant_entries"]) == (1, 1, 0, 1, 3)


def test_precision_divides_by_the_cutoff_not_by_the_list_length():
    e, v = one_list([10, 20], {20: 5.0}, 10)
    assert v["hits"] == 1 and e["hits"][0] / 10 == 0.1 and v["recall"] == 1.0 and v["rr"] == 0.5
    assert v["ap"] == 0.5                                             # (1 / 2) / min(|R| = 1, 10)


def test_fewer_relevant_items_than_the_cutoff():
    e, v = one_list([1, 2, 3, 4, 5], {1: 5.0, 2: 5.0}, 5)
    assert v == {"hits": 2.0, "recall": 1.0, "ap": 1.0, "rr": 1.0, "ndcg": 1.0}      # IDCG takes min(N, |R|) terms
    e, v = one_list([3, 1, 2], {1: 5.0, 2: 5.0}, 3)
    assert v["ap"] == pytest.approx((1 / 2 + 2 / 3) / 2, rel=1e-15)
    assert v["ndcg"] == pytest.approx((1 / math.log2(3) + 1 / 2) / (1 + 1 / math.log2(3)), rel=1e-15)


def test_graded_gains():
    R = {20: 2.0, 40: 5.0, 99: 3.0, 50: 1.0}          # 50: below the threshold of 2, no gain and not in |R_u|
    e, v = one_list([10, 20, 30, 40], R, 4, "linear", 2.0)
    assert e["relevant_entries"] == 3 and v["recall"] == pytest.approx(2 / 3, rel=1e-15)
    assert v["ndcg"] == pytest.approx((2 / math.log2(3) + 5 / math.log2(5)) / (5 + 3 / math.log2(3) + 2 / 2), rel=1e-15)
    e, v = one_list([10, 20, 30, 40], R, 4, "exp2", 2.0)
    assert v["ndcg"] == pytest.approx((3 / math.log2(3) + 31 / math.log2(5)) / (31 + 7 / math.log2(3) + 3 / 2), rel=1e-15)
    e, v = one_list([10, 20, 30, 40], R, 1, "exp2", 2.0)
    assert v["ndcg"] == 0.0 and v["hits"] == 0.0 and v["rr"] == 0.0


def test_threshold_nan_duplicates_and_lists_without_relevant_items():
    test = (np.array([1, 1, 2, 3], dtype=np.int32), np.array([5, 6, 5, 5], dtype=np.int32), np.array([4.0, np.nan, 3.5, 4.0], dtype=np.float32))
    lu, li = np.array([1, 1, 2, 4], dtype=np.int32), np.array([6, 5, 5, 5], dtype=np.int32)
    e = eval_ref.evaluate(lu, li, test, (1, 2), 4.0, coverage=True)
    assert (e["lists"], e["users_evaluated"], e["lists_without_relevant"], e["relevant_users"], e["relevant_entries"]) == (3, 1, 2, 2, 2)
    assert e["hits"] == [0, 1] and e["users_hit"] == [0, 1] and e["rr"] == [0.0, 0.5] and e["distinct_items"] == 2
    assert np.isnan(e["per_user"]["hits"][1:]).all() and list(e["per_user"]["user"]) == [1, 2, 4]
    with pytest.raises(ValueError):
        eval_ref.evaluate(lu, li, (test[0][[0, 0]], test[1][[0, 0]], test[2][[0, 0]]), (1,), 4.0)


def test_an_item_named_twice_counts_twice():
    e, v = one_list([20, 20, 30], {20: 5.0}, 3)
    assert v["hits"] == 2 and v["recall"] == 2.0


def test_struct_sizes_and_abi_version():
    P = pkg()
    P.build()
    assert C.sizeof(P._native.EvalParams) == 56
    assert C.sizeof(P._native.EvalSums) == 480
    assert P._native.EvalSums.ms.offset == 472 and P._native.EvalParams.relevance_threshold.offset == 48
    assert P._native.load().fy_abi_version() == 5


def test_the_split_of_the_golden_fixture(rm_golden):
    u, i, s = rm_golden["coo"]
    keep = s > 0
    u, i, s = u[keep], i[keep], s[keep]
    assert len(u) == 2489
    (tu, ti, ts), (eu, ei, es) = eval_ref.holdout(u, i, s, 0.2, 1)
    assert len(eu) == 507 and len(tu) == 2489 - 507
    m = eval_ref.split_mask(u, i, 0.2, 1)
    assert np.array_equal(eu, u[m]) and np.array_equal(ti, i[~m])                     # source order on both sides
    assert set(np.unique(tu).tolist()) == set(range(1, 31))
    assert set(np.unique(eu[es >= 4]).tolist()) == set(range(1, 31))
    # the key alone decides: another order, another neighbourhood, the same side
    order = np.random.default_rng(0).permutation(len(u))
    assert np.array_equal(eval_ref.split_mask(u[order], i[order], 0.2, 1), m[order])
    assert not np.array_equal(eval_ref.split_mask(u, i, 0.2, 2), m)
    assert not eval_ref.split_mask(u, i, 0.0, 1).any() and eval_ref.split_mask(u, i, 1.0, 1).all()
