"""Estimated preferences for named pairs: the statement (tests/estimate_ref.py) against the CPU oracle of item-based CF on the
reference's own fixture, the layouts of the new ABI structs, the NULL refusals and the means of EstimateErrors.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import estimate_ref as ER
import oracle
from test_itemcf_gpu import RTOL
from util import pkg

assert RTOL == 2e-6


def golden(rm_golden):
    u, i, s = rm_golden["coo"]
    keep = (s > 0) & (u != 7) & (i != 13)
    return u[keep], i[keep], s[keep]


@pytest.mark.parametrize("boolean", [False, True])
@pytest.mark.parametrize("max_prefs,K", [(8, 20), (50, 10)])
def test_the_statement_is_the_oracles_cell(rm_golden, max_prefs, K, boolean):
    u, i, s = golden(rm_golden)
    sims = oracle.itemsim(u, i, s, max_similarities_per_item=K)
    ref = oracle.itemcf(u, i, s, sims["item"], sims["other"], sims["sim"], num_recommendations=1 << 30, max_prefs_per_user=max_prefs,
                        boolean_data=boolean)
    users, items = np.unique(u), np.unique(i)
    gu, gi = (a.ravel() for a in np.meshgrid(users, items, indexing="ij"))
    value, status = ER.estimate(u, i, s, sims["item"], sims["other"], sims["sim"], gu, gi, max_prefs, boolean)
    cell = {(int(a), int(b)): (v, st) for a, b, v, st in zip(gu, gi, value, status)}
    assert len(ref["user"]) > 100
    for a, b, sc in zip(ref["user"].tolist(), ref["item"].tolist(), ref["score"].tolist()):
        v, st = cell[(a, b)]
        assert st == ER.OK and abs(float(np.float32(v)) - sc) <= RTOL * abs(sc), (a, b, v, sc, st)
    in_oracle = set(zip(ref["user"].tolist(), ref["item"].tolist()))
    assert {k for k, (_, st) in cell.items() if st == ER.OK} == in_oracle          # every cell that is not OK is absent from the oracle
    assert np.isnan(value[status != ER.OK]).all() and not np.isnan(value[status == ER.OK]).any()
    assert (status == ER.OWN_PREFERENCE).any() and (status == ER.TOO_FEW).any()
    # unknown ids come first
    v, st = ER.estimate(u, i, s, sims["item"], sims["other"], sims["sim"], [7, 7, 1, -1, 2 ** 31 - 1], [13, 1, 13, 1, 1], max_prefs, boolean)
    assert st.tolist() == [ER.UNKNOWN_USER, ER.UNKNOWN_USER, ER.UNKNOWN_ITEM, ER.UNKNOWN_USER, ER.UNKNOWN_USER] and np.isnan(v).all()


def test_hand_cells():
    # three users; item 3 is in the rows of items 1 and 2
    u = np.array([1, 1, 2, 2, 2, 3], dtype=np.int32)
    i = np.array([1, 2, 1, 2, 3, 3], dtype=np.int32)
    s = np.array([4.0, 2.0, 5.0, 1.0, 3.0, 2.0], dtype=np.float32)
    sim_item, sim_other, sim_value = [1, 1, 2, 2, 3], [2, 3, 1, 3, 1], [0.5, 0.25, 0.5, -0.75, 0.25]
    v, st = ER.estimate(u, i, s, sim_item, sim_other, sim_value, [1, 1, 1, 3, 3, 2], [3, 1, 2, 1, 3, 3], 50)
    assert st.tolist() == [ER.OK, ER.OWN_PREFERENCE, ER.OWN_PREFERENCE, ER.TOO_FEW, ER.OWN_PREFERENCE, ER.OWN_PREFERENCE]
    assert v[0] == (4.0 * 0.25 + 2.0 * -0.75) / (0.25 + 0.75)
    # maxPrefs 1: user 1 keeps item 1 alone; item 2, rated below the cut, is an ordinary cell with one contribution
    v, st = ER.estimate(u, i, s, sim_item, sim_other, sim_value, [1, 1, 1], [1, 2, 3], 1)
    assert st.tolist() == [ER.OWN_PREFERENCE, ER.TOO_FEW, ER.TOO_FEW]
    v, st = ER.estimate(u, i, s, sim_item, sim_other, sim_value, [1, 1, 1], [1, 2, 3], 1, boolean=True)
    assert st.tolist() == [ER.OWN_PREFERENCE, ER.OK, ER.OK] and v.tolist()[1:] == [0.5, 0.25]
    # +1 and -1 on items that are equally similar to the target: the numerator is exactly 0
    s2 = np.array([1.0, -1.0, 5.0, 1.0, 3.0, 2.0], dtype=np.float32)
    v, st = ER.estimate(u, i, s2, sim_item, [2, 3, 1, 3, 1], [0.5, 0.25, 0.5, 0.25, 0.25], [1], [3], 50)
    assert st.tolist() == [ER.ZERO_NUMERATOR]
    assert ER.row_entries_walked(u, i, s, sim_item, [1, 1, 2, 9], [3, 1, 3, 3], 50, 1) == 2 * 4 + 1 * 5
    assert ER.row_entries_walked(u, i, s, sim_item, [1, 1, 2, 9], [3, 1, 3, 3], 50, 2) == 4 + 5


def test_error_sums_by_hand():
    e = ER.errors([3.5, 6.0, np.nan, 2.0, 1.0], [0, 0, 4, 0, 0], [4.0, 5.0, 3.0, np.nan, 1.5])
    assert (e["pairs"], e["estimated"], e["truth_not_finite"]) == (5, 3, 1) and e["by_status"][:5] == [4, 0, 0, 0, 1]
    assert e["abs"] == [0.5, 1.0, 0.5] and e["sq"] == [0.25, 1.0, 0.25] and e["err"] == [-0.5, 1.0, -0.5]
    e = ER.errors([3.5, 6.0, np.nan, 2.0, 1.0], [0, 0, 4, 0, 0], [4.0, 5.0, 3.0, np.nan, 1.5], clamp=(1.5, 5.0))
    assert e["err"] == [-0.5, 0.0, 0.0] and e["estimated"] == 3


def test_struct_sizes_and_abi_version():
    P = pkg()
    P.build()
    N = P._native
    assert C.sizeof(N.ItemCFPairs) == 32 and N.ItemCFPairs.location.offset == 24
    assert C.sizeof(N.ItemCFEstimateStats) == 160 and N.ItemCFEstimateStats.row_entries_walked.offset == 152
    assert N.ItemCFEstimateStats.by_status.offset == 16 and N.ItemCFEstimateStats.users_known.offset == 80
    assert C.sizeof(N.EvalErrorParams) == 24 and N.EvalErrorParams.clamp_lo.offset == 8
    assert C.sizeof(N.EvalErrors) == 120 and N.EvalErrors.sum_abs.offset == 88 and N.EvalErrors.ms.offset == 112
    assert N.load().fy_abi_version() == 5
    assert (P.FY_ESTIMATE_OK, P.FY_ESTIMATE_UNKNOWN_USER, P.FY_ESTIMATE_UNKNOWN_ITEM, P.FY_ESTIMATE_OWN_PREFERENCE, P.FY_ESTIMATE_TOO_FEW,
            P.FY_ESTIMATE_ZERO_NUMERATOR, P.FY_ESTIMATE_NOT_A_NUMBER) == tuple(range(7))
    assert (ER.OK, ER.UNKNOWN_USER, ER.UNKNOWN_ITEM, ER.OWN_PREFERENCE, ER.TOO_FEW, ER.ZERO_NUMERATOR, ER.NOT_A_NUMBER) == tuple(range(7))


def test_null_arguments_without_a_device():
    P = pkg()
    N = P._native
    lib = N.load()
    out = C.c_void_p(1)
    prm, pairs = N.ItemCFParams(0, 50, 0, 0, 1, 0), N.ItemCFPairs(0, None, None, 0)
    assert lib.fy_itemcf_estimate_prepared(None, C.byref(prm), C.byref(pairs), C.byref(out)) == -1 and not out.value
    assert b"NULL" in lib.fy_last_error()
    assert lib.fy_itemcf_estimate_prepared(None, C.byref(prm), C.byref(pairs), None) == -1
    out = C.c_void_p(1)
    assert lib.fy_itemcf_estimate_ratings(None, C.byref(prm), None, C.byref(out)) == -1 and not out.value
    assert lib.fy_result_itemcf_estimate_stats(None, C.byref(N.ItemCFEstimateStats())) == -1
    assert lib.fy_eval_estimates(None, None, None, None, C.byref(N.EvalErrors())) == -1


def test_estimate_errors_means_and_merge():
    P = pkg()
    a = P.EstimateErrors(10, 4, 1, [5, 1, 1, 2, 1, 0, 0, 0], 2.0, 1.5, -1.0, 0.25)
    assert (a.mae, a.rmse, a.bias, a.coverage) == (0.5, math.sqrt(0.375), -0.25, 0.4)
    b = P.EstimateErrors(6, 2, 0, [2, 0, 0, 4, 0, 0, 0, 0], 1.0, 0.5, 1.0, 0.5)
    m = P.EstimateErrors.merge([a, b])
    assert (m.pairs, m.estimated, m.truth_not_finite, m.by_status) == (16, 6, 1, [7, 1, 1, 6, 1, 0, 0, 0])
    assert (m.sum_abs, m.sum_sq, m.sum_err, m.ms) == (3.0, 2.0, 0.0, 0.75)
    assert (m.mae, m.rmse, m.bias, m.coverage) == (0.5, math.sqrt(2.0 / 6), 0.0, 6 / 16)
    nothing = P.EstimateErrors(3, 0, 0, [0, 3, 0, 0, 0, 0, 0, 0], 0.0, 0.0, 0.0)
    assert math.isnan(nothing.mae) and math.isnan(nothing.rmse) and nothing.coverage == 0.0
    assert math.isnan(P.EstimateErrors(0, 0, 0, [0] * 8, 0.0, 0.0, 0.0).coverage)
    with pytest.raises(ValueError):
        P.EstimateErrors.merge([])
