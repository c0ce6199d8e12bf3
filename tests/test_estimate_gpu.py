"""Estimated preferences for named pairs on a prepared similarity job (fy_itemcf_estimate_prepared / _ratings) and their error
sums (fy_eval_estimates).

The main yardstick is the list pass itself: wherever a list of ``prepared.recommend`` holds (user, item), the estimate is that float
BIT FOR BIT, and every other pair of the grid carries the status tests/estimate_ref.py (numpy / fp64, fed with the job's own rows)
gives it.  For all seven measures the CPU oracle of item-based CF (oracle/itemcf_oracle.c), fed with the job's rows, is compared at
the RTOL of the existing item-CF tests (imported, not restated).  The error sums are compared with math.fsum over the reference's
per-pair terms within 4 n 2^-53 sum |term| (n ordered fp64 additions, slack 4).

Shapes: golden 30 x 100 integers N 5 maxPrefs 8 K 20; tiny 200 x 300 half stars N 10 maxPrefs 10 K 15; ml100k 943 x 1682 maxPrefs 50
K 100 (a row longer than a wave) where it is named."""
import ctypes as C
import math

import numpy as np
import pytest

import estimate_ref as ER
import itemsim_measures_ref as MR
from test_itemcf_filter_gpu import bits, dataset, oracle_full, user_request
from test_itemcf_gpu import RTOL
from test_itemcf_request_gpu import BITWISE, SHAPES
from util import pkg

pytestmark = pytest.mark.gpu
assert RTOL == 2e-6


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


def est_bits(rows):
    return list(zip(rows["user"].tolist(), rows["item"].tolist(), rows["estimate"].view(np.uint32).tolist(), rows["status"].tolist()))


def grid_of(users, items):
    gu, gi = (a.ravel().astype(np.int32) for a in np.meshgrid(users, items, indexing="ij"))
    return gu, gi


def job_rows(prepared, i):
    r = prepared.rows(np.unique(i)).rows()
    return r["item"], r["other"], r["sim"].astype(np.float64)


def check_grid_against_the_lists(prepared, u, i, s, users, o, boolean):
    """every pair of users x all items: in a list -> status 0 and the list's bits; else the reference's status != 0"""
    items = np.unique(i)
    assert len(items) <= 2048
    rec = prepared.recommend(users, numRecommendations=len(items), maxPrefsPerUser=o["max_prefs"], booleanData=boolean)
    lists = {(a, b): c for a, b, c in bits(rec.rows())}
    gu, gi = grid_of(users, items)
    est = prepared.estimate((gu, gi), maxPrefsPerUser=o["max_prefs"], booleanData=boolean)
    rows = est.rows()
    assert est.size == len(gu) and np.array_equal(rows["user"], gu) and np.array_equal(rows["item"], gi)
    _, want_status = ER.estimate(u, i, s, *job_rows(prepared, i), gu, gi, o["max_prefs"], boolean)
    got_bits, got_status = rows["estimate"].view(np.uint32), rows["status"]
    in_list = np.array([(a, b) in lists for a, b in zip(gu.tolist(), gi.tolist())])
    want_bits = np.array([lists.get((a, b), 0) for a, b in zip(gu.tolist(), gi.tolist())], dtype=np.uint32)
    assert len(lists) > 100 and in_list.sum() == len(lists)
    assert (got_status[in_list] == 0).all() and np.array_equal(got_bits[in_list], want_bits[in_list])
    assert (got_status[~in_list] != 0).all() and np.array_equal(got_status[~in_list], want_status[~in_list])
    assert np.isnan(rows["estimate"][~in_list]).all()
    assert (got_status == 3).any() and (got_status == 4).any()
    st = est.estimate_stats
    assert st["pairs_asked"] == len(gu) and st["pair_offset"] == 0 and st["by_status"] == [int((got_status == q).sum()) for q in range(8)]
    assert st["users_known"] == len(np.intersect1d(users, u)) and st["targets"] == st["users_known"] * len(items)
    assert est.stats["recs"] == est.size and est.stats["users_scored"] == len({a for a, _ in lists}) == rec.stats["users_scored"]
    assert est.stats["ms_prepare"] == 0 and est.stats["ms_topn"] == 0 and est.stats["nnz"] == len(u)
    return rows


# ------------------------------------------------------------------------------------------------ 1. bitwise the lists
@pytest.mark.parametrize("boolean", [False, True])
@pytest.mark.parametrize("shape", ["golden", "tiny"])
@pytest.mark.parametrize("measure", BITWISE)
def test_bitwise_the_lists(ctx, rm_golden, measure, shape, boolean):
    u, i, s = dataset(shape, rm_golden)
    o = SHAPES[shape]
    prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=measure)
    check_grid_against_the_lists(prepared, u, i, s, np.unique(u), o, boolean)
    prepared.close()


def test_bitwise_the_lists_rows_longer_than_a_wave(ctx):
    u, i, s = dataset("ml100k", None)
    o = SHAPES["ml100k"]
    assert o["K"] > 64
    prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.COSINE)
    check_grid_against_the_lists(prepared, u, i, s, np.unique(u)[::19][:50], o, False)
    prepared.close()


# ------------------------------------------------------------------------------------------------ 2. against the oracle
@pytest.mark.parametrize("shape", ["golden", "tiny"])
@pytest.mark.parametrize("measure", MR.MEASURES)
def test_against_the_oracle_fed_with_the_jobs_rows(ctx, rm_golden, measure, shape):
    u, i, s = dataset(shape, rm_golden)
    o = SHAPES[shape]
    users = user_request(u, np.random.default_rng(5))
    prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=measure)
    ref = oracle_full(u, i, s, prepared.rows(np.unique(i)), o["max_prefs"], False)
    gu, gi = grid_of(users, np.unique(i))
    rows = prepared.estimate((gu, gi), maxPrefsPerUser=o["max_prefs"]).rows()
    prepared.close()
    asked = np.isin(ref["user"], users)
    want = {(a, b): c for a, b, c in zip(ref["user"][asked].tolist(), ref["item"][asked].tolist(), ref["score"][asked].tolist())}
    ok = rows["status"] == 0
    compared = set()
    for a, b, v in zip(rows["user"][ok].tolist(), rows["item"][ok].tolist(), rows["estimate"][ok].tolist()):
        assert abs(v - want[(a, b)]) <= RTOL * abs(want[(a, b)]), (a, b, v, want[(a, b)])
        compared.add((a, b))
    assert compared == set(want) and len(want) > 100          # the status-0 set is the oracle's set of cells; no row is left uncompared
    assert np.isnan(rows["estimate"][~ok]).all()


# ------------------------------------------------------------------------------------------------ 3. the awkward requests
def test_awkward_requests(ctx, rm_golden):
    u, i, s = dataset("golden", rm_golden)
    o = SHAPES["golden"]
    prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"])
    sims = job_rows(prepared, i)
    # a user with more preferences than maxPrefs: items at the cut (tie kept) and below it
    heavy = next(x for x in np.unique(u).tolist() if (u == x).sum() > o["max_prefs"] and (s[u == x] < np.sort(s[u == x])[::-1][o["max_prefs"] - 1]).any())
    p, it = s[u == heavy], i[u == heavy]
    cut = np.sort(p)[::-1][o["max_prefs"] - 1]
    at_cut, below = it[p == cut], it[p < cut]
    assert len(at_cut) > 0 and len(below) > 0 and (p >= cut).sum() > o["max_prefs"]          # a tie at the cut is kept
    known_items = np.unique(i)
    pairs = [(heavy, int(x)) for x in at_cut] + [(heavy, int(x)) for x in below]
    pairs += [(3, int(x)) for x in known_items[:40]] + [(3, 13), (3, 0), (3, 101), (3, -5), (3, 2 ** 31 - 1), (3, -2 ** 31)]
    pairs += [(7, 1), (31, 1), (0, 1), (-4, 1), (2 ** 31 - 1, 1), (-2 ** 31, 1), (7, 13), (-4, 13)]
    pairs += [(3, int(known_items[5]))] * 3 + [(heavy, int(below[0]))] * 2                   # duplicates
    pairs += [(x, int(y)) for x in (1, 2, 5, 30) for y in known_items[::9]]
    order = np.random.default_rng(2).permutation(len(pairs))                                 # one user's pairs scattered through the input
    pu = np.array([pairs[k][0] for k in order], dtype=np.int64).astype(np.int32)
    pi = np.array([pairs[k][1] for k in order], dtype=np.int64).astype(np.int32)
    value, status = ER.estimate(u, i, s, *sims, pu, pi, o["max_prefs"])
    at = {(a, b): st for a, b, st in zip(pu.tolist(), pi.tolist(), status.tolist())}
    assert all(at[(heavy, int(x))] == 3 for x in at_cut) and all(at[(heavy, int(x))] != 3 for x in below)
    assert {at[(7, 1)], at[(-4, 13)], at[(2 ** 31 - 1, 1)], at[(-2 ** 31, 1)]} == {1} and {at[(3, 13)], at[(3, 101)], at[(3, -2 ** 31)]} == {2}
    assert set(status.tolist()) >= {0, 1, 2, 3}
    est = prepared.estimate((pu, pi), maxPrefsPerUser=o["max_prefs"])
    rows = est.rows()
    assert np.array_equal(rows["user"], pu) and np.array_equal(rows["item"], pi)            # the order asked, duplicates answered
    assert np.array_equal(rows["status"], status)
    ok = status == 0
    np.testing.assert_allclose(rows["estimate"][ok], value[ok], rtol=RTOL)
    assert np.isnan(rows["estimate"][~ok]).all()
    seen = {}
    for row in est_bits(rows):                                                               # equal pairs, equal rows
        assert seen.setdefault(row[:2], row) == row
    assert est.estimate_stats["targets"] == len({k for k, st in at.items() if st not in (1, 2)}) < len(pairs)
    # one pair on its own; a device request; no pair at all
    k = int(np.flatnonzero(ok)[0])
    one = prepared.estimate((pu[k:k + 1], pi[k:k + 1]), maxPrefsPerUser=o["max_prefs"])
    assert est_bits(one.rows()) == est_bits(rows)[k:k + 1] and one.estimate_stats["chunks"] == 1
    import torch
    dev = prepared.estimate((torch.from_numpy(pu).cuda(), torch.from_numpy(pi).cuda()), maxPrefsPerUser=o["max_prefs"])
    assert est_bits(dev.rows()) == est_bits(rows)
    empty = np.zeros(0, dtype=np.int32)
    none = prepared.estimate((empty, empty))
    assert none.size == 0 and len(none.rows()["user"]) == 0 and none.estimate_stats["by_status"] == [0] * 8 and none.stats["users_scored"] == 0
    unknown = prepared.estimate(([7, -1], [1, 13]))
    assert unknown.rows()["status"].tolist() == [1, 1] and unknown.estimate_stats["users_known"] == 0 and unknown.estimate_stats["rows_built"] == 0
    prepared.close()
    z = np.zeros(0, dtype=np.int32)
    nothing = pkg().BaselineRecommenderJob(ctx).prepare((z, z, np.zeros(0, dtype=np.float32)))
    assert nothing.estimate(([1, 2], [3, 4])).rows()["status"].tolist() == [1, 1]
    nothing.close()


# ------------------------------------------------------------------------------------------------ 4. chunking
def test_chunks_change_no_bit(ctx, monkeypatch):
    u, i, s = dataset("tiny", None)
    o = SHAPES["tiny"]
    items = np.arange(1, 301, dtype=np.int32)          # the catalogue; one of its items has no rating in `tiny`
    n_known = len(np.unique(i))
    assert n_known == 299 and np.isin(i, items).all()
    prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"])
    sim_item = prepared.rows(items).rows()["item"]
    gu, gi = grid_of(np.unique(u), items)
    whole = prepared.estimate((gu, gi), maxPrefsPerUser=o["max_prefs"])
    user = int(np.unique(u)[17])
    pu, pi = np.full(len(items), user, dtype=np.int32), items[::-1].astype(np.int32)
    want = {r[:2]: r for r in est_bits(whole.rows()) if r[0] == user}
    assert len(want) == 300 and any(r[3] == 0 for r in want.values()) and sum(r[3] == 2 for r in want.values()) == 1
    base = prepared.estimate((pu, pi), maxPrefsPerUser=o["max_prefs"])
    monkeypatch.setenv("FY_ICF_EST_CHUNK", "4")
    forced = prepared.estimate((pu, pi), maxPrefsPerUser=o["max_prefs"])
    monkeypatch.delenv("FY_ICF_EST_CHUNK")
    assert est_bits(forced.rows()) == est_bits(base.rows()) == [want[(user, int(b))] for b in pi]
    for est, chunk in ((base, 256), (forced, 4)):
        st = est.estimate_stats
        assert st["targets"] == n_known and st["chunks"] == -(-n_known // chunk)
        assert st["row_entries_walked"] == ER.row_entries_walked(u, i, s, sim_item, pu, pi, o["max_prefs"], chunk) > 0
    assert whole.estimate_stats["row_entries_walked"] == ER.row_entries_walked(u, i, s, sim_item, gu, gi, o["max_prefs"], 256)
    prepared.close()


# ------------------------------------------------------------------------------------------------ 5. zero numerator
def test_a_numerator_of_exactly_zero(ctx):
    X, Y, T, Z = 10, 20, 30, 40
    u = np.array([1, 1, 2, 2, 3, 3, 4, 4, 4], dtype=np.int32)
    i = np.array([X, Y, X, T, Y, T, X, Y, Z], dtype=np.int32)
    raw = np.array([4, 2, 4, 4, 4, 4, 5, 5, 5], dtype=np.float32)
    shift = -3.0
    s = (raw + np.float32(shift)).astype(np.float32)
    assert s[0] == 1.0 and s[1] == -1.0
    # co-occurrence similarity by hand: the number of users who rated both
    ids = np.unique(i)
    rated = {int(a): set(u[i == a].tolist()) for a in ids}
    sim = [(int(a), int(b), float(len(rated[int(a)] & rated[int(b)]))) for a in ids for b in ids if a != b and rated[int(a)] & rated[int(b)]]
    si, so, sv = (np.array(c) for c in zip(*sim))
    assert dict(((a, b), v) for a, b, v in sim)[(X, T)] == dict(((a, b), v) for a, b, v in sim)[(Y, T)] == 1.0
    pu, pi = np.array([1, 1, 1, 1, 4], dtype=np.int32), np.array([T, Z, X, 99, T], dtype=np.int32)
    value, status = ER.estimate(u, i, s, si, so, sv, pu, pi, 50)
    assert status[0] == ER.ZERO_NUMERATOR                     # the construction, before the GPU is asked
    assert status.tolist() == [5, 5, 3, 2, 0] and value[4] == (2.0 * 1 + 2.0 * 1) / (1 + 1)
    prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, raw), maxSimilaritiesPerItem=20, similarityClassname=MR.COOCCURRENCE, ratingShift=shift)
    r = prepared.rows(ids).rows()
    assert sorted(zip(r["item"].tolist(), r["other"].tolist(), r["sim"].tolist())) == sorted(sim)
    rows = prepared.estimate((pu, pi)).rows()
    assert rows["status"].tolist() == status.tolist() and rows["status"][0] == 5 and np.isnan(rows["estimate"][0])
    ok = status == 0
    np.testing.assert_allclose(rows["estimate"][ok], value[ok], rtol=RTOL)
    # the list pass drops the same cell
    lists = prepared.recommend([1], numRecommendations=10).rows()
    assert T not in lists["item"].tolist()
    prepared.close()


# ------------------------------------------------------------------------------------------------ 6. the store
def test_the_row_store_changes_no_estimate(ctx):
    P = pkg()
    u, i, s = dataset("tiny", None)
    o = SHAPES["tiny"]
    users = np.unique(u)[5:40]
    gu, gi = grid_of(users, np.unique(i)[::3])
    kw = dict(maxPrefsPerUser=o["max_prefs"])
    job = P.BaselineRecommenderJob(ctx)
    prepared = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.LOGLIKELIHOOD)
    cold = prepared.estimate((gu, gi), **kw)
    st = cold.estimate_stats
    assert st["rows_built"] == st["items_needed"] == st["rows_stored"] > 0 and st["rows_from_store"] == 0 and st["batches"] >= 1
    assert st["pair_contribs"] == cold.stats["pair_contribs"] > 0
    want = est_bits(cold.rows())
    assert any(r[3] == 0 for r in want)
    warm = prepared.estimate((gu, gi), **kw)
    q = warm.estimate_stats
    assert q["rows_built"] == 0 and q["pair_contribs"] == 0 and q["batches"] == 0 and q["rows_from_store"] == st["items_needed"]
    assert est_bits(warm.rows()) == want
    # a later recommend finds every row of these users in the store
    rec = prepared.recommend(users, numRecommendations=o["N"], **kw)
    assert rec.request_stats["rows_built"] == 0 and rec.request_stats["rows_from_store"] == st["items_needed"] and rec.size > 0
    prepared.drop_rows()
    again = prepared.estimate((gu, gi), **kw)
    assert again.estimate_stats["rows_built"] == st["items_needed"] and est_bits(again.rows()) == want
    prepared.close()
    # a store filled by recommend for the same users
    fresh = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.LOGLIKELIHOOD)
    rec2 = fresh.recommend(users, numRecommendations=o["N"], **kw)
    assert rec2.request_stats["rows_built"] == st["items_needed"] and bits(rec2.rows()) == bits(rec.rows())
    served = fresh.estimate((gu, gi), **kw)
    assert served.estimate_stats["rows_from_store"] == st["items_needed"] > 0 and served.estimate_stats["rows_built"] == 0
    assert est_bits(served.rows()) == want
    fresh.close()


# ------------------------------------------------------------------------------------------------ 7. + 8. hold-out, errors, ranks
@pytest.fixture(scope="module")
def split(ctx):
    """tiny, 20 % held out: the prepared job on the train side, the resident test side, both sides on the host, the reference"""
    P = pkg()
    u, i, s = dataset("tiny", None)
    o = SHAPES["tiny"]
    R = P.Ratings(ctx, u, i, s)
    train, test = R.holdout(0.2, seed=3)
    R.close()
    prepared = P.BaselineRecommenderJob(ctx).prepare(train, maxSimilaritiesPerItem=o["K"])
    tu, ti, ts = train.to_host()
    eu, ei, es = test.to_host()
    value, status = ER.estimate(tu, ti, ts, *job_rows(prepared, ti), eu, ei, o["max_prefs"])
    yield dict(prepared=prepared, test=test, test_host=(eu, ei, es), value=value, status=status, max_prefs=o["max_prefs"])
    prepared.close()
    test.close()
    train.close()


def check_sums(err, ref):
    for name, terms in (("sum_abs", ref["abs"]), ("sum_sq", ref["sq"]), ("sum_err", ref["err"])):
        want, bound = math.fsum(terms), ER.sum_bound(terms)
        print(name, getattr(err, name), "reference", want, "bound", bound)
        assert abs(getattr(err, name) - want) <= bound, name


def counters(e):
    return (e.pairs, e.estimated, e.truth_not_finite, e.by_status)


def test_errors_on_a_hold_out(ctx, split):
    P = pkg()
    prepared, test, (eu, ei, es) = split["prepared"], split["test"], split["test_host"]
    est = prepared.estimate(test, maxPrefsPerUser=split["max_prefs"])          # a resident Ratings: nothing is downloaded
    rows = est.rows()
    assert np.array_equal(rows["user"], eu) and np.array_equal(rows["item"], ei) and np.array_equal(rows["status"], split["status"])
    ok = rows["status"] == 0
    np.testing.assert_allclose(rows["estimate"][ok], split["value"][ok], rtol=RTOL)
    err = est.errors(test)
    ref = ER.errors(rows["estimate"], rows["status"], es)
    assert counters(err) == (ref["pairs"], ref["estimated"], ref["truth_not_finite"], ref["by_status"])
    assert err.estimated >= 50 and err.estimated == ok.sum() and err.truth_not_finite == 0 and err.pairs == len(eu) == test.nnz
    check_sums(err, ref)
    assert err.mae == err.sum_abs / err.estimated and err.rmse == math.sqrt(err.sum_sq / err.estimated) and 0 < err.coverage < 1
    again = est.errors(test)
    assert (again.sum_abs.hex(), again.sum_sq.hex(), again.sum_err.hex()) == (err.sum_abs.hex(), err.sum_sq.hex(), err.sum_err.hex())
    # a clamp into the rating scale: the same rows, other terms
    clamped = est.errors(test, clamp=(0.5, 5))
    cref = ER.errors(rows["estimate"], rows["status"], es, clamp=(0.5, 5))
    assert counters(clamped) == counters(err)
    check_sums(clamped, cref)
    tight = est.errors(test, clamp=(3, 3.5))
    check_sums(tight, ER.errors(rows["estimate"], rows["status"], es, clamp=(3, 3.5)))
    assert tight.sum_abs != err.sum_abs
    for bad in ((5, 0.5), (float("nan"), 5), (0.5, float("nan"))):
        with pytest.raises(P.FilmYouError) as e:
            est.errors(test, clamp=bad)
        assert e.value.code == -1
    # a truth with one pair swapped, a shorter truth
    k = int(np.flatnonzero(ok)[0])
    j = k + 1 if (eu[k + 1], ei[k + 1]) != (eu[k], ei[k]) else k + 2
    order = np.arange(len(eu))
    order[[k, j]] = order[[j, k]]
    for wrong in (P.Ratings(ctx, eu[order], ei[order], es[order]), P.Ratings(ctx, eu[:-1], ei[:-1], es[:-1])):
        with pytest.raises(P.FilmYouError) as e:
            est.errors(wrong)
        assert e.value.code == -1
        wrong.close()
    # a NaN truth score on an OK row
    es2 = es.copy()
    es2[k] = np.nan
    holed = P.Ratings(ctx, eu, ei, es2)
    e2 = est.errors(holed)
    assert e2.truth_not_finite == 1 and e2.estimated == err.estimated - 1 and e2.by_status == err.by_status
    check_sums(e2, ER.errors(rows["estimate"], rows["status"], es2))
    holed.close()


def test_ranks_cut_the_pair_list(ctx, split):
    P = pkg()
    prepared, test = split["prepared"], split["test"]
    kw = dict(maxPrefsPerUser=split["max_prefs"])
    whole = prepared.estimate(test, **kw)
    parts = [prepared.estimate(test, rank=r, world=3, **kw) for r in range(3)]
    n = whole.size
    assert [p.estimate_stats["pair_offset"] for p in parts] == [n * r // 3 for r in range(3)] and sum(p.size for p in parts) == n
    assert [row for p in parts for row in est_bits(p.rows())] == est_bits(whole.rows())
    # host pairs cut the same way
    eu, ei, es = split["test_host"]
    host = [prepared.estimate((eu, ei), rank=r, world=3, **kw) for r in range(3)]
    assert [est_bits(p.rows()) for p in host] == [est_bits(p.rows()) for p in parts]
    e_whole = whole.errors(test)
    merged = P.EstimateErrors.merge([p.errors(test) for p in parts])
    assert counters(merged) == counters(e_whole) and merged.estimated >= 50
    rows = whole.rows()
    check_sums(merged, ER.errors(rows["estimate"], rows["status"], es))
    with pytest.raises(RuntimeError, match=r"BaselineRecommenderJob failed!.*rank"):
        prepared.estimate(test, rank=3, world=3)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(ctx, rm_golden, split):
    P = pkg()
    u, i, s = dataset("golden", rm_golden)
    for bad, what in ((dict(world=2), "world"), (dict(minPrefsPerUser=2), "minPrefsPerUser")):
        other = P.RowSimilarityJob(ctx).prepare((u, i, s), maxSimilaritiesPerRow=20, **bad)
        with pytest.raises(RuntimeError, match=r"BaselineRecommenderJob failed!.*" + what) as e:
            other.estimate(([1, 2], [3, 4]))
        assert e.value.__cause__.code == -10          # FY_ERR_UNSUPPORTED
        other.close()
    prepared, test = split["prepared"], split["test"]
    with pytest.raises(RuntimeError, match="maxPrefsPerUser") as e:
        prepared.estimate(test, maxPrefsPerUser=0)
    assert e.value.__cause__.code == -1
    with pytest.raises(ValueError):
        prepared.estimate(([2 ** 31], [1]))
    est = prepared.estimate(test, maxPrefsPerUser=split["max_prefs"])
    ev = P.Evaluator(ctx, test, cutoffs=(5,), relevance_threshold=4.0)
    with pytest.raises(P.FilmYouError) as e:
        ev.evaluate(est)
    assert e.value.code == -1                         # FY_ERR_INVALID_ARGUMENT
    ev.close()
    with pytest.raises(RuntimeError) as e:
        P.BaselineRecommenderJob(ctx).run(test, similarities=est)
    assert e.value.__cause__.code == -1
    # and a list result is no estimates result
    rec = prepared.recommend(np.unique(split["test_host"][0])[:5], numRecommendations=5)
    out = P._native.EvalErrors()
    assert P._native.load().fy_eval_estimates(ctx._h, rec._h, test._h, None, C.byref(out)) == -1
    assert P._native.load().fy_result_itemcf_estimate_stats(rec._h, C.byref(P._native.ItemCFEstimateStats())) == -9          # FY_ERR_STATE
