"""Item-based lists for given profiles and pending writes on a prepared similarity job (fy_itemcf_recommend_profiles).

Three yardsticks.  (1) A profile that composes to a resident row must get that user's list of ``prepared.recommend`` BITWISE: the pass
behind the ingest is the same code over the same rows.  (2) Writes applied on a resident row must give, bitwise, the list of the merged
profile handed in whole, with the merge made by the plain statement tests/profile_ref.py -- and every counter of
fy_itemcf_profile_stats is that statement's count.  (3) For all seven measures, profiles of users the job was NOT prepared on are
compared with profile_ref's lists computed from the job's own rows (prepared.rows(all items)) through `compare` of the existing
item-CF tests at their RTOL = 2e-6 (imported, not restated), which asserts that no row was left out.

Shapes: golden 30 x 100 integers N 5 maxPrefs 8 K 20; tiny 200 x 300 half stars N 10 maxPrefs 10 K 15; ml100k (test 1 only) N 20
maxPrefs 50 K 100; the widths test builds its own 1200-item catalogue so that one profile composes to more than 1024 preferences."""
import ctypes as C

import numpy as np
import pytest

import itemsim_measures_ref as MR
import profile_ref as PR
from test_itemcf_filter_gpu import bits, compare, dataset, item_request, user_request
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


def by_user(rows):
    """{user: its rows' bits, in order}"""
    out = {}
    for row in bits(rows):
        out.setdefault(row[0], []).append(row)
    return out


def in_profile_order(rows, labels):
    groups = by_user(rows)
    return [row for x in labels for row in groups.get(int(x), [])]


def row_of(u, i, s, x, rng=None):
    m = u == x
    it, sc = i[m], s[m]
    if rng is not None:
        order = rng.permutation(len(it))
        it, sc = it[order], sc[order]
    return it, sc


# ------------------------------------------------------------------------------------------------ 1. a resident row given whole
@pytest.mark.parametrize("boolean", [False, True])
@pytest.mark.parametrize("shape", ["golden", "tiny", "ml100k"])
@pytest.mark.parametrize("measure", BITWISE)
def test_a_resident_row_given_whole_is_that_users_list(ctx, rm_golden, measure, shape, boolean):
    P = pkg()
    u, i, s = dataset(shape, rm_golden)
    o = SHAPES[shape]
    rng = np.random.default_rng(11)
    users, items = user_request(u, rng), item_request(i, rng)
    kw = dict(numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"], booleanData=boolean)
    prepared = P.BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=measure)
    labels = rng.permutation(np.intersect1d(users, u))          # the known requested users once each, in no particular order
    profiles = [(int(x),) + row_of(u, i, s, x, rng) for x in labels]
    for extra in (dict(), dict(itemsFile=items)):
        want = prepared.recommend(users, **extra, **kw)
        expected = in_profile_order(want.rows(), labels)
        assert len(expected) == want.size > 0
        whole = prepared.recommend_profiles(profiles, base="whole", **extra, **kw)
        assert bits(whole.rows()) == expected, (measure, shape, extra.keys())
        ps = whole.profile_stats
        assert ps["profiles_asked"] == ps["profiles_mine"] == len(labels) and ps["profiles_scored"] == want.stats["users_scored"] == whole.stats["users_scored"]
        assert ps["prefs_composed"] == ps["entries"] == int(np.isin(u, labels).sum()) and ps["profiles_empty"] == 0 and ps["users_unknown"] == 0
        assert whole.stats["recs"] == whole.size == want.size
        # the resident row with nothing applied, unknown ids among the labels
        asked = np.concatenate([labels, [-3, int(u.max()) + 1, 2 ** 31 - 1]]).astype(np.int32)
        resident = prepared.recommend_profiles([(int(x), [], []) for x in asked], base="resident", **extra, **kw)
        assert bits(resident.rows()) == expected
        ps = resident.profile_stats
        assert ps["users_unknown"] == ps["profiles_empty"] == 3 and ps["entries"] == 0 and ps["prefs_composed"] == int(np.isin(u, labels).sum())
    # two ranks together are the one rank's rows
    parts = [prepared.recommend_profiles(profiles, base="whole", rank=r, world=2, **kw) for r in range(2)]
    assert [row for p in parts for row in bits(p.rows())] == in_profile_order(prepared.recommend(users, **kw).rows(), labels)
    assert [p.profile_stats["profiles_mine"] for p in parts] == [len(labels) // 2, len(labels) - len(labels) // 2]
    assert all(p.size > 0 for p in parts)
    prepared.close()


# ------------------------------------------------------------------------------------------------ 2. writes on a resident row
def writes_for(u, i, s, x, rank, unknown_item):
    """(items, scores, remove) for user x: an upsert of an existing item, a new item, deletes of the first and the last entry of the row,
    a delete of an absent item, an item written three times (delete, write, write: the last wins), an unknown item, a negative id"""
    it, _ = row_of(u, i, s, x)
    row = sorted(it.tolist(), key=lambda a: rank[a])
    absent = [a for a in sorted(rank, key=lambda a: rank[a]) if a not in set(row)]
    assert len(row) >= 4 and len(absent) >= 3
    new, gone, twice = absent[0], absent[1], absent[2]
    w = [(row[len(row) // 2], 0.5, 0), (new, 4.5, 0), (row[0], 9.0, 1), (row[-1], 9.0, 1), (gone, 1.0, 1), (twice, 2.0, 1), (twice, 1.5, 0),
         (unknown_item, 3.0, 0), (-5, 3.0, 0), (twice, 3.5, 0), (unknown_item, 0.0, 1)]
    return [a for a, _, _ in w], [b for _, b, _ in w], [c for _, _, c in w]


@pytest.mark.parametrize("boolean", [False, True])
@pytest.mark.parametrize("shape", ["golden", "tiny"])
def test_writes_on_a_resident_row_match_the_merged_profile(ctx, rm_golden, shape, boolean):
    P = pkg()
    u, i, s = dataset(shape, rm_golden)
    o = SHAPES[shape]
    kw = dict(numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"], booleanData=boolean)
    rank = PR.popularity_rank(i)
    unknown_item = 13 if shape == "golden" else int(i.max()) + 7
    assert unknown_item not in rank
    known = np.unique(u)
    labels = [int(x) for x in known[[1, 4, 9, 16, 22]]] + [int(known.max()) + 3]          # the last one: a user the job does not know
    profiles = [(x,) + tuple(writes_for(u, i, s, x if x in known else labels[0], rank, unknown_item)) for x in labels]
    prepared = P.BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.LOGLIKELIHOOD)
    got = prepared.recommend_profiles(profiles, base="resident", **kw)
    composed, want_c = PR.compose(u, i, s, profiles, "resident")
    merged = [(x, [a for a, _ in prefs], [b for _, b in prefs]) for x, prefs in composed]
    whole = prepared.recommend_profiles(merged, base="whole", **kw)
    assert got.size > 0 and bits(got.rows()) == bits(whole.rows())
    assert len(by_user(got.rows())) >= 5
    ps = got.profile_stats
    print(ps)
    for k in PR.COUNTERS:
        assert ps[k] == want_c[k], (k, ps[k], want_c[k])
    assert ps["profiles_scored"] == len(by_user(got.rows())) == got.stats["users_scored"]
    assert ps["removes_hit"] == 10 and ps["removes_missed"] == 8 and ps["entries_superseded"] == 12 and ps["users_unknown"] == 1
    assert ps["entries_unknown_item"] == 18 and ps["entries"] == 66
    assert whole.profile_stats["prefs_composed"] == ps["prefs_composed"] == whole.profile_stats["entries"]
    # the writes changed the lists
    before = prepared.recommend(np.array(labels, dtype=np.int32), **kw)
    assert bits(before.rows()) != bits(got.rows())
    prepared.close()


# ------------------------------------------------------------------------------------------------ 3. against the plain statement
@pytest.mark.parametrize("shape", ["golden", "tiny"])
@pytest.mark.parametrize("measure", MR.MEASURES)
def test_profiles_of_users_the_job_does_not_know_against_the_statement(ctx, rm_golden, measure, shape):
    P = pkg()
    u, i, s = dataset(shape, rm_golden)
    assert (s > 0).all()
    o = SHAPES[shape]
    known = np.unique(u)
    half = np.isin(u, known[::2])
    ua, ia, sa = u[half], i[half], s[half]
    rng = np.random.default_rng(5)
    strangers = known[1::2]
    profiles = [(int(x),) + row_of(u, i, s, x, rng) + (None,) for x in strangers]
    prepared = P.BaselineRecommenderJob(ctx).prepare((ua, ia, sa), maxSimilaritiesPerItem=o["K"], similarityClassname=measure)
    sims = prepared.rows(np.unique(ia)).rows()
    composed, want_c = PR.compose(ua, ia, sa, [(x, a.tolist(), b.tolist(), None) for x, a, b, _ in profiles], "whole")
    ref = PR.lists(composed, sims["item"], sims["other"], sims["sim"], o["max_prefs"])
    rec = prepared.recommend_profiles([p[:3] for p in profiles], numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"])
    rows = compare(rec, ref, o["N"])
    assert len(rows["user"]) > 0
    assert [x for x in strangers.tolist() if x in set(rows["user"].tolist())] == list(dict.fromkeys(rows["user"].tolist()))      # the order given
    for k in PR.COUNTERS:
        assert rec.profile_stats[k] == want_c[k], k
    items = item_request(ia, rng)
    rec_b = prepared.recommend_profiles([p[:3] for p in profiles], numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"], itemsFile=items)
    compare(rec_b, PR.lists(composed, sims["item"], sims["other"], sims["sim"], o["max_prefs"], allow=items), o["N"])
    prepared.close()


# ------------------------------------------------------------------------------------------------ 4. widths
WIDTHS = [0, 1, 2, 63, 64, 65, 127, 129, 1100]


@pytest.fixture(scope="module")
def wide(ctx):
    """1200 items, 60 users of 80 items each and one who rated everything; cosine K 10.  -> (ratings, prepared job, its rows)"""
    rng = np.random.default_rng(77)
    items = np.arange(1, 1201, dtype=np.int32) * 3
    u = [np.full(80, 10 + x, dtype=np.int32) for x in range(60)] + [np.full(len(items), 5, dtype=np.int32)]
    i = [rng.choice(items, size=80, replace=False) for _ in range(60)] + [items]
    u, i = np.concatenate(u), np.concatenate(i).astype(np.int32)
    s = (rng.integers(1, 11, size=len(u)) / 2.0).astype(np.float32)
    prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=10, similarityClassname=MR.COSINE)
    sims = prepared.rows(items).rows()
    yield (u, i, s), prepared, sims
    prepared.close()


def wide_profiles(items, rng):
    """300 whole profiles labelled 5000 ..: the first ones compose to the WIDTHS (the widest by writing every item twice, the last write
    winning), then one with a tie exactly at the maxPrefs = 10 cut, then random ones of 0 .. 40 preferences with a few deletes"""
    out = []
    for w in WIDTHS:
        pick = rng.choice(items, size=w, replace=False)
        sc = (rng.integers(1, 11, size=w) / 2.0).astype(np.float32)
        if w > 1024:
            out.append((pick.tolist() * 2, np.concatenate([np.full(w, 0.5, dtype=np.float32), sc]).tolist(), [0] * (2 * w)))
        else:
            out.append((pick.tolist(), sc.tolist(), [0] * w))
    pick = rng.choice(items, size=14, replace=False)
    out.append((pick.tolist(), [5.0] * 9 + [4.0] * 3 + [3.0] * 2, [0] * 14))          # the 10th largest is 4.0: twelve are kept
    while len(out) < 300:
        n = int(rng.integers(0, 41))
        pick = rng.choice(items[:200], size=n)          # with repeats
        out.append((pick.tolist(), (rng.integers(1, 11, size=n) / 2.0).tolist(), (rng.random(n) < 0.1).astype(np.uint8).tolist()))
    return [(5000 + p,) + t for p, t in enumerate(out)]


def test_widths_at_which_the_ingest_can_go_wrong(ctx, wide):
    (u, i, s), prepared, sims = wide
    rng = np.random.default_rng(3)
    profiles = wide_profiles(np.unique(i), rng)
    kw = dict(numRecommendations=10, maxPrefsPerUser=10)
    composed, want_c = PR.compose(u, i, s, profiles, "whole")
    assert [len(prefs) for _, prefs in composed[:len(WIDTHS)]] == WIDTHS
    assert len(PR.kept(composed[len(WIDTHS)][1], 10)) == 12
    all300 = prepared.recommend_profiles(profiles, **kw)
    for k in PR.COUNTERS:
        assert all300.profile_stats[k] == want_c[k], (k, all300.profile_stats[k], want_c[k])
    assert want_c["profiles_empty"] >= 1 and want_c["entries_superseded"] >= 1100 and want_c["removes_missed"] > 0
    ref = PR.lists(composed, sims["item"], sims["other"], sims["sim"], 10)
    rows = compare(all300, ref, 10)
    groups = by_user(rows)
    assert list(groups) == [x for x, _ in composed if x in groups]          # grouped by profile in the order given
    assert 5000 + len(WIDTHS) - 1 in groups and len(groups) >= 10          # the widest profile and many others got a list
    # two runs are bit-identical
    assert bits(prepared.recommend_profiles(profiles, **kw).rows()) == bits(rows)
    # one profile alone, five profiles, the three hundred: the same bits per profile
    five = prepared.recommend_profiles(profiles[:5], **kw)
    assert five.profile_stats["profiles_asked"] == 5 and bits(five.rows()) == [r for x, _ in composed[:5] for r in groups.get(x, [])]
    for p in (3, len(WIDTHS) - 1, len(WIDTHS), 200):
        alone = prepared.recommend_profiles(profiles[p:p + 1], **kw)
        assert alone.profile_stats["profiles_asked"] == 1 and bits(alone.rows()) == groups.get(5000 + p, []), p
    # the same widths on top of a resident row: user 5 rated everything, the entries delete all but w items of the row
    heavy_items = np.unique(i)
    res_profiles = [(5, heavy_items[w:].tolist(), [0.0] * (len(heavy_items) - w), [1] * (len(heavy_items) - w)) for w in (0, 1, 64, 65, 1100)]
    res = prepared.recommend_profiles(res_profiles, base="resident", **kw)
    comp_r, want_r = PR.compose(u, i, s, res_profiles, "resident")
    assert [len(prefs) for _, prefs in comp_r] == [0, 1, 64, 65, 1100]
    for k in PR.COUNTERS:
        assert res.profile_stats[k] == want_r[k], k
    merged = prepared.recommend_profiles([(x, [a for a, _ in prefs], [b for _, b in prefs]) for x, prefs in comp_r], **kw)
    assert res.size > 0 and bits(res.rows()) == bits(merged.rows())          # (the label repeats: four groups of user 5 in the order given)


# ------------------------------------------------------------------------------------------------ 5. the store
def test_the_store_is_shared_and_changes_no_result(ctx):
    P = pkg()
    u, i, s = dataset("tiny", None)
    o = SHAPES["tiny"]
    kw = dict(numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"])
    users = np.unique(u)[:12]
    rng = np.random.default_rng(9)
    profiles = [(int(x),) + row_of(u, i, s, x, rng) for x in users]
    job = P.BaselineRecommenderJob(ctx)
    prepared = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.LOGLIKELIHOOD)
    cold = prepared.recommend_profiles(profiles, **kw)
    q = cold.profile_stats
    assert cold.size > 0 and q["rows_built"] == q["items_needed"] == q["rows_stored"] > 0 and q["rows_from_store"] == 0 and q["batches"] >= 1
    assert q["pair_contribs"] == cold.stats["pair_contribs"] > 0
    warm = prepared.recommend_profiles(profiles, **kw)
    w = warm.profile_stats
    assert w["rows_built"] == 0 and w["batches"] == 0 and w["pair_contribs"] == 0 and w["rows_from_store"] == w["items_needed"] == q["items_needed"]
    assert bits(warm.rows()) == bits(cold.rows())
    # rows built by recommend_profiles are found by recommend and estimate
    rec = prepared.recommend(users, **kw)
    assert rec.request_stats["rows_built"] == 0 and rec.request_stats["rows_from_store"] == q["items_needed"]
    assert in_profile_order(rec.rows(), users) == bits(cold.rows())
    est = prepared.estimate((users, np.full(len(users), int(i[0]), dtype=np.int32)), maxPrefsPerUser=o["max_prefs"])
    assert est.estimate_stats["rows_built"] == 0 and est.estimate_stats["rows_from_store"] > 0
    prepared.drop_rows()
    again = prepared.recommend_profiles(profiles, **kw)
    assert again.profile_stats["rows_built"] == q["rows_built"] and again.profile_stats["rows_from_store"] == 0 and bits(again.rows()) == bits(cold.rows())
    prepared.close()
    # the other way round: rows built by recommend serve recommend_profiles
    fresh = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.LOGLIKELIHOOD)
    assert fresh.recommend(users, **kw).request_stats["rows_built"] == q["rows_built"]
    after = fresh.recommend_profiles(profiles, **kw)
    assert after.profile_stats["rows_built"] == 0 and after.profile_stats["rows_from_store"] == q["items_needed"] and bits(after.rows()) == bits(cold.rows())
    fresh.close()


# ------------------------------------------------------------------------------------------------ 6. the evaluator takes the result
def test_the_evaluator_takes_the_result(ctx):
    P = pkg()
    u, i, s = dataset("tiny", None)
    o = SHAPES["tiny"]
    known = np.unique(u)
    half = np.isin(u, known[::2])
    prepared = P.BaselineRecommenderJob(ctx).prepare((u[half], i[half], s[half]), maxSimilaritiesPerItem=o["K"])
    rng = np.random.default_rng(2)
    # the strangers' profiles are a part of their ratings; the rest is the test side
    profiles, test = [], []
    for x in known[1::2][:40]:
        it, sc = row_of(u, i, s, x, rng)
        cut = len(it) // 2
        profiles.append((int(x), it[:cut], sc[:cut]))
        test.append((np.full(len(it) - cut, x, dtype=np.int32), it[cut:], sc[cut:]))
    T = P.Ratings(ctx, *(np.concatenate([t[k] for t in test]) for k in range(3)))
    E = P.Evaluator(ctx, T, cutoffs=(5, 10), relevance_threshold=3.0, coverage=True)
    rec = prepared.recommend_profiles(profiles, numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"])
    rows = rec.rows()
    a, b = E.evaluate(rec), E.evaluate(P.ItemRecommendations.from_rows(ctx, rows["user"], rows["item"], rows["score"]))
    assert a.lists == rec.profile_stats["profiles_scored"] > 0
    for k in P.Evaluation.COUNTERS:
        assert getattr(a, k) == getattr(b, k), k
    assert np.array_equal(a.hits, b.hits) and np.array_equal(a.users_hit, b.users_hit) and a.distinct_items == b.distinct_items
    for k in P.Evaluation.SUMS:
        assert np.array_equal(getattr(a, k).view(np.int64), getattr(b, k).view(np.int64)), k
    E.close()
    T.close()
    prepared.close()


# ------------------------------------------------------------------------------------------------ 7. edges and failures
def test_edges(ctx, rm_golden):
    P = pkg()
    u, i, s = dataset("golden", rm_golden)
    o = SHAPES["golden"]
    job = P.BaselineRecommenderJob(ctx)
    kw = dict(numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"])
    prepared = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"])
    empty = np.zeros(0, dtype=np.int32)
    cases = (([], "whole", {}), ([(1, [], []), (2, [], [])], "whole", {}), ([(7, [], []), (-4, [13, -1], [1.0, 2.0])], "resident", {}),
             ([(1, [], [])], "resident", dict(itemsFile=empty)), ([(1, [1, 2, 1, 2], [1.0, 2.0, 0.0, 0.0], [0, 0, 1, 1])], "whole", {}))
    for profiles, base, extra in cases:
        rec = prepared.recommend_profiles(profiles, base=base, **extra, **kw)
        assert rec.size == 0 and rec.stats["recs"] == 0 and rec.stats["users_scored"] == 0 and len(rec.rows()["user"]) == 0
        ps = rec.profile_stats
        assert ps["profiles_asked"] == len(profiles) and ps["rows_built"] == 0 and ps["profiles_scored"] == 0 and ps["prefs_composed"] == 0
        assert ps["profiles_empty"] == len(profiles) or "itemsFile" in extra
    assert prepared.recommend_profiles([(1, [], [])], base="resident", **kw).size > 0
    # a repeated label: two groups in the order given, each the list of its own variant
    it1, sc1 = row_of(u, i, s, 1)
    n1 = len(it1)
    assert n1 >= 40
    a, b, c = (5, it1[:n1 // 2], sc1[:n1 // 2]), (9, it1[n1 // 4:3 * n1 // 4], sc1[n1 // 4:3 * n1 // 4]), (5, it1[n1 // 3:], sc1[n1 // 3:])
    three = prepared.recommend_profiles([a, b, c], **kw).rows()
    alone = [bits(prepared.recommend_profiles([p], **kw).rows()) for p in (a, b, c)]
    assert all(len(x) > 0 for x in alone) and bits(three) == alone[0] + alone[1] + alone[2]
    assert [x for x in dict.fromkeys(three["user"].tolist())] == [5, 9] and three["user"].tolist() == [5] * len(alone[0]) + [9] * len(alone[1]) + [5] * len(alone[2])
    assert alone[0] != alone[2]
    with pytest.raises(ValueError):
        prepared.recommend_profiles(None)
    prepared.close()
    # a job over no preferences
    z = np.zeros(0, dtype=np.int32)
    nothing = job.prepare((z, z, np.zeros(0, dtype=np.float32)))
    rec = nothing.recommend_profiles([(1, [1, 2], [3.0, 4.0])])
    assert rec.size == 0 and rec.profile_stats["profiles_asked"] == 1 and rec.profile_stats["profiles_mine"] == 0
    nothing.close()


def test_rating_shift_feeds_a_shifted_job_raw_scores(ctx):
    P = pkg()
    u, i, s = dataset("tiny", None)
    o = SHAPES["tiny"]
    kw = dict(numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"])
    users = np.unique(u)[[3, 50, 120]]
    prepared = P.BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"], ratingShift=-0.5)
    want = prepared.recommend(users, **kw)
    rng = np.random.default_rng(1)
    profiles = [(int(x),) + row_of(u, i, s, x, rng) for x in users]
    got = prepared.recommend_profiles(profiles, ratingShift=-0.5, **kw)
    assert want.size > 0 and bits(got.rows()) == in_profile_order(want.rows(), users)
    assert bits(prepared.recommend_profiles(profiles, **kw).rows()) != bits(got.rows())          # unshifted scores are other preferences
    prepared.close()


def raw_call(prepared, n, user, start, item, score, remove, base, has_users=0, N=5):
    """fy_itemcf_recommend_profiles through ctypes with arrays the Python layer would refuse -> (status, message)"""
    Nv = pkg()._native
    lib = Nv.load()
    ptr = lambda a: None if a is None else a.ctypes.data
    prm = Nv.ItemCFParams(N, 8, 0, 0, 1, 0)
    q = Nv.ItemCFProfiles(n, ptr(user), ptr(start), ptr(item), ptr(score), ptr(remove), base)
    f = Nv.ItemCFFilter(has_users, 0, 0, None, 0, None)
    out = C.c_void_p(1)
    rc = lib.fy_itemcf_recommend_profiles(prepared._h, C.byref(prm), C.byref(q), C.byref(f), C.byref(out))
    assert rc != 0 and not out.value
    return rc, lib.fy_last_error().decode()


def test_failures_leave_a_usable_job(ctx, rm_golden):
    """Every bad input here is one the host refuses before any launch."""
    P = pkg()
    u, i, s = dataset("golden", rm_golden)
    o = SHAPES["golden"]
    kw = dict(numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"])
    job = P.BaselineRecommenderJob(ctx)
    prepared = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"])
    users = np.unique(u)[:10]
    profiles = [(int(x),) + row_of(u, i, s, x) for x in users]
    want = in_profile_order(prepared.recommend(users, **kw).rows(), users)
    assert len(want) > 0
    lab, st, it, sc = np.array([1, 2], dtype=np.int32), np.array([0, 1, 2], dtype=np.int64), np.array([1, 2], dtype=np.int32), np.array([1.0, 2.0], dtype=np.float32)
    INVALID, UNSUPPORTED = -1, -10
    assert raw_call(prepared, 2, None, st, it, sc, None, 0)[0] == INVALID          # NULL arrays with n_profiles > 0
    assert raw_call(prepared, 2, lab, None, it, sc, None, 0)[0] == INVALID
    assert raw_call(prepared, 2, lab, st, None, sc, None, 0)[0] == INVALID
    assert raw_call(prepared, 2, lab, st, it, None, None, 0)[0] == INVALID
    assert raw_call(prepared, 2, lab, np.array([0, 2, 1], dtype=np.int64), it, sc, None, 0)[0] == INVALID          # start decreases
    assert raw_call(prepared, 2, lab, np.array([1, 1, 2], dtype=np.int64), it, sc, None, 0)[0] == INVALID          # start does not begin at 0
    assert raw_call(prepared, 2, lab, st, it, sc, None, 2)[0] == INVALID and raw_call(prepared, 2, lab, st, it, sc, None, -1)[0] == INVALID
    assert raw_call(prepared, 2, lab, st, it, sc, None, 0, has_users=1)[0] == INVALID
    assert raw_call(prepared, -1, lab, st, it, sc, None, 0)[0] == INVALID
    rc, msg = raw_call(prepared, 2, lab, np.array([0, 1, 2 ** 31], dtype=np.int64), it, sc, None, 0)          # refused on the offsets alone
    assert rc == UNSUPPORTED and "2^31" in msg
    assert raw_call(prepared, 2, lab, st, it, sc, None, 0, N=0)[0] == INVALID and raw_call(prepared, 2, lab, st, it, sc, None, 0, N=4096)[0] == UNSUPPORTED
    for n, what in ((0, "numRecommendations must be > 0"), (4096, "2048")):
        with pytest.raises(RuntimeError, match=r"BaselineRecommenderJob failed!.*" + what):
            prepared.recommend_profiles(profiles, numRecommendations=n)
    with pytest.raises(RuntimeError, match=r"BaselineRecommenderJob failed!.*rank"):
        prepared.recommend_profiles(profiles, rank=2, world=2)
    # after the failed calls the job answers as before, cold and warm
    assert bits(prepared.recommend_profiles(profiles, **kw).rows()) == want
    assert bits(prepared.recommend_profiles(profiles, **kw).rows()) == want
    # an allocation that fails half way: the call fails, the job and its store stay usable
    failed = 0
    for n in (2, 9, 17):
        ctx.inject_alloc_failure(n)
        try:
            prepared.recommend_profiles(profiles[::-1], base="resident", **kw)
        except RuntimeError as e:
            assert e.__cause__.code == -4, e
            failed += 1
        finally:
            ctx.inject_alloc_failure(0)
    assert failed >= 2
    assert bits(prepared.recommend_profiles(profiles, **kw).rows()) == want
    prepared.close()
    # jobs this pass cannot serve
    for bad, what in ((dict(world=2), "world"), (dict(maxPrefsPerUser=5), "maxPrefsPerUser")):
        other = P.RowSimilarityJob(ctx).prepare((u, i, s), maxSimilaritiesPerRow=o["K"], **bad)
        with pytest.raises(RuntimeError, match=r"BaselineRecommenderJob failed!.*" + what) as e:
            other.recommend_profiles(profiles, **kw)
        assert e.value.__cause__.code == UNSUPPORTED
        assert other.rows(np.unique(i)).size > 0
        other.close()
