"""Item-based recommendations on request from a prepared similarity job (fy_itemcf_recommend_prepared).

Two yardsticks.  Where the request's similarity rows are bitwise the full build's (half stars, integers; every measure but
Pearson) the lists must be BITWISE those of today's path, BaselineRecommenderJob.run(similarities=full matrix, usersFile=...),
whose code the request path shares from the thresholds on.  For all seven measures the CPU oracle of item-based CF
(oracle/itemcf_oracle.c) is fed with the job's own rows -- prepared.rows(all items) -- and restricted to the request, through
`check` / `compare` of the existing item-CF tests at their RTOL = 2e-6 (imported, not restated); `compare` asserts that no row
was left out of the comparison.  The request statistics are counted again in numpy from the ratings: the kept preferences of a
user are those >= its maxPrefs-th largest value (all when it has no more than that), J is their union over the known requested
users, walk[j] = sum over the raters v of j of n_v.

Shapes (both cuts bite): golden 30 x 100 integers N 5 maxPrefs 8 K 20; tiny 200 x 300 half stars N 10 maxPrefs 10 K 15; ml100k
943 x 1682 integers N 20 maxPrefs 50 K 100."""
import numpy as np
import pytest

import itemsim_measures_ref as MR
from test_itemcf_filter_gpu import bits, compare, dataset, item_request, oracle_full, restrict, user_request
from test_itemcf_gpu import RTOL
from util import pkg

pytestmark = pytest.mark.gpu
assert RTOL == 2e-6
SHAPES = {"golden": dict(N=5, max_prefs=8, K=20), "tiny": dict(N=10, max_prefs=10, K=15), "ml100k": dict(N=20, max_prefs=50, K=100)}
BITWISE = [MR.COSINE, MR.COOCCURRENCE, MR.TANIMOTO, MR.LOGLIKELIHOOD]


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


def needed_items(u, i, s, users, max_prefs):
    """-> (known requested users, J): the items among the kept (strongest) preferences of the known requested users"""
    J, known = set(), []
    for x in np.unique(users).tolist():
        m = u == x
        if not m.any():
            continue
        known.append(x)
        p, it = s[m], i[m]
        if len(p) > max_prefs:
            it = it[p >= np.sort(p)[::-1][max_prefs - 1]]
        J.update(it.tolist())
    return known, np.array(sorted(J), dtype=np.int32)


def walk_sum(u, i, items):
    deg = np.bincount(u)
    return int(deg[u[np.isin(i, items)]].astype(np.int64).sum())


def cold_stats(rec, u, i, s, users, max_prefs):
    """the statistics of a request on a cold store count the work"""
    known, J = needed_items(u, i, s, users, max_prefs)
    rq = rec.request_stats
    print(rq, "|J|", len(J), "known users", len(known))
    assert rq["users_asked"] == len(users) and rq["users_known"] == len(known)
    assert rq["items_needed"] == len(J) > 0
    assert rq["rows_built"] == len(J) == rq["rows_stored"] and rq["rows_from_store"] == 0
    assert rq["pair_contribs"] == rec.stats["pair_contribs"] == walk_sum(u, i, J)
    assert rq["batches"] == rec.stats["cooc_launches"] >= 1
    assert rec.stats["ms_prepare"] == 0 and rec.stats["nnz"] == len(u)
    assert rec.stats["n_users"] == len(np.unique(u)) and rec.stats["n_items"] == len(np.unique(i))
    return J


# ------------------------------------------------------------------------------------------------ 1. bitwise today's answer
@pytest.mark.parametrize("boolean", [False, True])
@pytest.mark.parametrize("shape", ["golden", "tiny", "ml100k"])
@pytest.mark.parametrize("measure", BITWISE)
def test_bitwise_the_filtered_pass_on_the_full_matrix(ctx, rm_golden, measure, shape, boolean):
    P = pkg()
    u, i, s = dataset(shape, rm_golden)
    o = SHAPES[shape]
    rng = np.random.default_rng(11)
    users, items = user_request(u, rng), item_request(i, rng)
    job = P.BaselineRecommenderJob(ctx)
    kw = dict(numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"], booleanData=boolean)
    R = P.Ratings(ctx, u, i, s)
    full = P.RowSimilarityJob(ctx).run(R, measure, o["K"], True, None)
    prepared = job.prepare(R, maxSimilaritiesPerItem=o["K"], similarityClassname=measure)
    for extra in (dict(), dict(itemsFile=items)):
        want = job.run(R, similarities=full, usersFile=users, **extra, **kw)[0]
        got = prepared.recommend(users, **extra, **kw)
        assert want.size > 0 and bits(got.rows()) == bits(want.rows()), (measure, shape, extra.keys())
        assert got.stats["recs"] == want.stats["recs"] == got.size
        assert got.stats["users_scored"] == want.stats["users_scored"]
        if not extra:
            cold_stats(got, u, i, s, users, o["max_prefs"])
    # two ranks together are the one rank's rows
    whole = prepared.recommend(users, itemsFile=items, **kw)
    parts = [prepared.recommend(users, itemsFile=items, rank=r, world=2, **kw) for r in range(2)]
    assert [row for p in parts for row in bits(p.rows())] == bits(whole.rows())
    assert sum(p.request_stats["users_known"] for p in parts) == whole.request_stats["users_known"]
    assert all(p.size > 0 for p in parts)
    prepared.close()
    R.close()


# ------------------------------------------------------------------------------------------------ 2. against the oracle
@pytest.mark.parametrize("shape", ["golden", "tiny"])
@pytest.mark.parametrize("measure", MR.MEASURES)
def test_against_the_oracle_fed_with_the_jobs_rows(ctx, rm_golden, measure, shape):
    P = pkg()
    u, i, s = dataset(shape, rm_golden)
    assert (s > 0).all()          # (the Euclidean distance needs positive preferences)
    o = SHAPES[shape]
    rng = np.random.default_rng(5)
    users, items = user_request(u, rng), item_request(i, rng)
    prepared = P.BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=measure)
    sims = prepared.rows(np.unique(i))
    ref = oracle_full(u, i, s, sims, o["max_prefs"], False)
    rec = prepared.recommend(users, numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"])
    rows = compare(rec, restrict(ref, users=users), o["N"])
    assert len(rows["user"]) > 0
    known, _ = needed_items(u, i, s, users, o["max_prefs"])
    assert rec.request_stats["users_known"] == len(known) >= rec.stats["users_scored"]
    rec_b = prepared.recommend(users, numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"], itemsFile=items)
    compare(rec_b, restrict(ref, users=users, items=items), o["N"])
    prepared.close()


# ------------------------------------------------------------------------------------------------ 3. + 4. the row store
@pytest.mark.parametrize("shape", ["tiny", "ml100k"])
def test_the_row_store_changes_no_result(ctx, shape):
    P = pkg()
    u, i, s = dataset(shape, None)
    o = SHAPES[shape]
    kw = dict(numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"])
    known = np.unique(u)
    users1, users2 = known[:12], known[6:30]
    prepared = P.BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.LOGLIKELIHOOD)
    ids = np.unique(i)[::7]
    rows_before = prepared.rows(ids)
    cold = prepared.recommend(users1, **kw)
    J1 = cold_stats(cold, u, i, s, users1, o["max_prefs"])
    assert cold.size > 0
    # the same request again: nothing is built
    warm = prepared.recommend(users1, **kw)
    q = warm.request_stats
    assert q["rows_built"] == 0 and q["pair_contribs"] == 0 and q["batches"] == 0 and q["rows_from_store"] == len(J1) == q["items_needed"]
    assert q["rows_stored"] == len(J1) and bits(warm.rows()) == bits(cold.rows())
    # an overlapping request builds exactly what is missing
    _, J2 = needed_items(u, i, s, users2, o["max_prefs"])
    new = np.setdiff1d(J2, J1)
    assert 0 < len(new) < len(J2)
    second = prepared.recommend(users2, **kw)
    q = second.request_stats
    assert q["items_needed"] == len(J2) and q["rows_built"] == len(new) and q["rows_from_store"] == len(J2) - len(new)
    assert q["pair_contribs"] == walk_sum(u, i, new) and q["rows_stored"] == len(np.union1d(J1, J2))
    # rows() neither reads nor fills the store
    rows_after = prepared.rows(ids)
    a, b = rows_before.rows(), rows_after.rows()
    assert len(a["item"]) > 0 and all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)
    assert rows_before.request_stats == rows_after.request_stats
    # a dropped store: everything is built again, the bits stay
    prepared.drop_rows()
    again = prepared.recommend(users1, **kw)
    assert again.request_stats["rows_built"] == len(J1) == again.request_stats["rows_stored"] and again.request_stats["rows_from_store"] == 0
    assert bits(again.rows()) == bits(cold.rows())
    fresh = P.BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.LOGLIKELIHOOD)
    assert bits(fresh.recommend(users2, **kw).rows()) == bits(second.rows())       # warm against cold
    fresh.close()
    prepared.close()


# ------------------------------------------------------------------------------------------------ 5. batches and chunks
@pytest.mark.parametrize("shape", ["tiny", "ml100k"])
def test_forced_chunks_and_batches_give_the_same_bits(ctx, monkeypatch, shape):
    P = pkg()
    u, i, s = dataset(shape, None)
    o = SHAPES[shape]
    kw = dict(numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"])
    users = user_request(u, np.random.default_rng({"tiny": 4, "ml100k": 3}[shape]), share=0.1)
    _, J = needed_items(u, i, s, users, o["max_prefs"])
    assert len(J) % 3 != 0      # (134 and 1382 rows: with three rows a batch the last batch is short)
    job = P.BaselineRecommenderJob(ctx)
    prepared = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.COSINE)
    base = prepared.recommend(users, **kw)
    prepared.close()
    assert base.size > 0 and base.request_stats["batches"] == 1
    monkeypatch.setenv("FY_ISIM_REQ_CHUNK", "256")      # several column chunks per row
    prepared = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.COSINE)
    monkeypatch.setenv("FY_ISIM_REQ_ROWS", "3")         # many batches, the last one short
    forced = prepared.recommend(users, **kw)
    chunks = prepared.rows(np.unique(i)[:1]).request_stats["chunks"]
    prepared.close()
    built = forced.request_stats["rows_built"]
    assert chunks == -(-len(np.unique(i)) // 256) > 1
    assert built == base.request_stats["rows_built"] == len(J) and forced.request_stats["batches"] == -(-built // 3) > 1
    assert bits(forced.rows()) == bits(base.rows())


# ------------------------------------------------------------------------------------------------ 6. after a write
@pytest.mark.parametrize("shift", [0.0, -0.5])
def test_after_a_write(ctx, shift):
    P = pkg()
    u, i, s = dataset("tiny", None)
    o = SHAPES["tiny"]
    known = np.unique(u)
    a, b, c = (int(x) for x in known[[3, 50, 120]])
    R = P.Ratings(ctx, u, i, s)
    ia, ib = i[u == a], i[u == b]
    new_item = int(np.setdiff1d(np.unique(i), i[u == c])[0])
    # an upsert to an existing key, a delete, an insert
    R2 = R.updated(np.array([a, b, c], dtype=np.int32), np.array([ia[0], ib[0], new_item], dtype=np.int32),
                   np.array([0.5, 0.0, 5.0], dtype=np.float32), remove=np.array([0, 1, 0], dtype=np.uint8))
    assert R2.update_stats["n_replaced"] == 1 and R2.update_stats["n_deleted"] == 1 and R2.update_stats["n_inserted"] == 1
    users = np.array([a, b, c], dtype=np.int32)
    job = P.BaselineRecommenderJob(ctx)
    kw = dict(numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"])
    stale = job.prepare(R, maxSimilaritiesPerItem=o["K"], ratingShift=shift)
    before = stale.recommend(users, **kw)
    want = job.run(R2, maxSimilaritiesPerItem=o["K"], usersFile=users, ratingShift=shift, **kw)[0]
    fresh = job.prepare(R2, maxSimilaritiesPerItem=o["K"], ratingShift=shift)
    got = fresh.recommend(users, **kw)
    assert want.size > 0 and bits(got.rows()) == bits(want.rows())
    assert bits(got.rows()) != bits(before.rows())
    stale.close()
    fresh.close()
    R.close()
    R2.close()


# ------------------------------------------------------------------------------------------------ 7. edges
def test_edges(ctx, rm_golden):
    P = pkg()
    u, i, s = dataset("golden", rm_golden)
    o = SHAPES["golden"]
    job = P.BaselineRecommenderJob(ctx)
    kw = dict(numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"])
    prepared = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"])
    empty = np.zeros(0, dtype=np.int32)
    for users, extra in ((empty, {}), ([1, 2], dict(itemsFile=empty)), ([7, 31, 0, -4, 2**31 - 1], {})):
        rec = prepared.recommend(users, **extra, **kw)
        assert rec.size == 0 and rec.stats["recs"] == 0 and rec.stats["users_scored"] == 0 and len(rec.rows()["user"]) == 0
        assert rec.request_stats["users_asked"] == len(users) and rec.request_stats["rows_built"] == 0
        assert rec.request_stats["users_known"] == 0 or "itemsFile" in extra
    with pytest.raises(ValueError):
        prepared.recommend(None)
    for n, what in ((0, "numRecommendations must be > 0"), (4096, "2048")):
        with pytest.raises(RuntimeError, match=r"BaselineRecommenderJob failed!.*" + what):
            prepared.recommend([1, 2], numRecommendations=n)
    assert prepared.recommend([1, 2], **kw).size > 0          # the job is as usable as before
    prepared.close()
    # a job over no preferences
    z = np.zeros(0, dtype=np.int32)
    nothing = job.prepare((z, z, np.zeros(0, dtype=np.float32)))
    rec = nothing.recommend([1, 2, 3])
    assert rec.size == 0 and rec.request_stats["users_asked"] == 3 and rec.request_stats["users_known"] == 0
    nothing.close()
    # a threshold no similarity reaches: every needed row is built and empty, nobody gets a list
    high = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"], threshold=2.0)
    users = np.unique(u)[:9]
    rec = high.recommend(users, **kw)
    _, J = needed_items(u, i, s, users, o["max_prefs"])
    assert rec.size == 0 and rec.stats["users_scored"] == 0 and rec.request_stats["rows_built"] == len(J) > 0
    assert high.recommend(users, **kw).request_stats["rows_from_store"] == len(J)
    high.close()
    # jobs this pass cannot serve
    for bad, what in ((dict(world=2), "world"), (dict(maxPrefsPerUser=5), "maxPrefsPerUser")):
        other = P.RowSimilarityJob(ctx).prepare((u, i, s), maxSimilaritiesPerRow=o["K"], **bad)
        with pytest.raises(RuntimeError, match=r"BaselineRecommenderJob failed!.*" + what) as e:
            other.recommend(users, **kw)
        assert e.value.__cause__.code == -10          # FY_ERR_UNSUPPORTED
        # and it still answers what it can (every item is asked for: with world = 2 the job owns the rows of even popularity rank only)
        assert other.rows(np.unique(i)).size > 0
        other.close()


# ------------------------------------------------------------------------------------------------ 8. a failed call leaves a usable job
def test_a_failed_call_leaves_a_usable_job(ctx, rm_golden):
    P = pkg()
    u, i, s = dataset("golden", rm_golden)
    o = SHAPES["golden"]
    kw = dict(numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"])
    job = P.BaselineRecommenderJob(ctx)
    users = np.unique(u)[:10]
    reference = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"])
    want = bits(reference.recommend(users, **kw).rows())
    reference.close()
    assert len(want) > 0
    prepared = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"])
    failed = succeeded = 0
    for n in range(1, 41):      # the n-th HBM request from now fails, until n is past the call's last request
        ctx.inject_alloc_failure(n)
        try:
            rec = prepared.recommend(users, **kw)
        except RuntimeError as e:
            assert e.__cause__.code == -4, e          # FY_ERR_OUT_OF_MEMORY
            failed += 1
            continue
        finally:
            ctx.inject_alloc_failure(0)
        assert bits(rec.rows()) == want
        succeeded += 1
        break
    print("failed calls", failed, "then succeeded", succeeded)
    assert failed > 5 and succeeded == 1          # a call with the injection armed ran to completion within the 40
    rec = prepared.recommend(users, **kw)
    assert bits(rec.rows()) == want
    prepared.drop_rows()
    assert bits(prepared.recommend(users, **kw).rows()) == want
    prepared.close()
