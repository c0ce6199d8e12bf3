"""Named pairs explained by their contributing preferences on a prepared similarity job (fy_itemcf_because_prepared).

Two yardsticks.  tests/because_ref.py (numpy / fp64, fed with the job's own rows): the listed rows -- pair, contributing item, the
bits of sim and pref -- are the reference's EXACTLY (the weight pref * sim is exact in fp64, so the order involves no rounding), and
so are the counts.  ``prepared.estimate`` of the same pairs: (estimate bits, status) per pair are equal bit for bit.

Shapes: golden 30 x 100 maxPrefs 8 K 20; tiny 200 x 300 half stars maxPrefs 10 K 15; ml100k 943 x 1682 K 100 (rows longer than a
wave); the crafted block of because_ref.block_data (75 contributors per target: more than lanes, more than how_many; a tie)."""
import ctypes as C

import numpy as np
import pytest

import because_ref as BR
import estimate_ref as ER
import itemsim_measures_ref as MR
from test_estimate_gpu import est_bits, grid_of
from test_itemcf_filter_gpu import dataset
from test_itemcf_request_gpu import BITWISE, SHAPES
from util import pkg

pytestmark = pytest.mark.gpu
HOW_MANY = (1, 3, 64)


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


def job_sims(prepared, i):
    r = prepared.rows(np.unique(i)).rows()
    return r["item"], r["other"], r["sim"]


def row_bits(bec):
    r = bec.rows()
    return list(zip(r["pair"].tolist(), r["because"].tolist(), r["sim"].view(np.uint32).tolist(), r["pref"].view(np.uint32).tolist()))


def pair_bits(bec):
    p = bec.pairs()
    return list(zip(p["user"].tolist(), p["item"].tolist(), p["estimate"].view(np.uint32).tolist(), p["status"].tolist()))


def everything(bec):
    p = bec.pairs()
    return row_bits(bec), pair_bits(bec), p["contributors"].tolist(), p["start"].tolist()


def check_against_reference(bec, allc, how_many, pu, pi):
    """rows, counts and starts of one call against the reference's contributors of the same pairs"""
    want_rows, want_cnt, want_start = BR.listed(allc, how_many)
    p, r = bec.pairs(), bec.rows()
    assert np.array_equal(p["user"], pu) and np.array_equal(p["item"], pi)                  # every pair once, in the order asked
    assert np.array_equal(p["contributors"], want_cnt)
    assert np.array_equal(np.diff(p["start"]), np.minimum(want_cnt, how_many))               # listed = min(contributors, how_many)
    assert np.array_equal(p["start"], want_start) and p["start"][0] == 0 and p["start"][-1] == bec.size == len(r["pair"])
    assert row_bits(bec) == want_rows
    assert np.array_equal(r["user"], pu[r["pair"]]) and np.array_equal(r["item"], pi[r["pair"]])
    st = bec.because_stats
    assert st["pairs_asked"] == len(pu) and st["rows"] == bec.size == bec.stats["recs"] and st["contributors"] == int(want_cnt.sum())
    assert st["by_status"] == [int((p["status"] == q).sum()) for q in range(8)]
    assert bec.stats["ms_prepare"] == 0 and bec.stats["ms_topn"] == 0


CASES = {}


def grid_case(ctx, rm_golden, measure, shape, boolean):
    """the grid users x all items of one (measure, shape, boolean): the three calls, the estimates and the reference, made once"""
    key = (measure, shape, boolean)
    if key not in CASES:
        u, i, s = dataset(shape, rm_golden)
        o = SHAPES[shape]
        prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=measure)
        gu, gi = grid_of(np.unique(u), np.unique(i))
        kw = dict(maxPrefsPerUser=o["max_prefs"], booleanData=boolean)
        allc = BR.contributors(u, i, s, *job_sims(prepared, i), gu, gi, o["max_prefs"], boolean)
        calls = {h: prepared.because((gu, gi), howMany=h, **kw) for h in HOW_MANY}
        est = prepared.estimate((gu, gi), **kw)
        CASES[key] = dict(data=(u, i, s), o=o, gu=gu, gi=gi, allc=allc, calls=calls, est=est_bits(est.rows()), est_stats=est.estimate_stats,
                          users_scored=est.stats["users_scored"])
        prepared.close()
    return CASES[key]


GRID = [pytest.param(m, sh, b, id="%s-%s-%s" % (m.rsplit(".", 1)[-1], sh, "boolean" if b else "prefs"))
        for m in BITWISE for sh in ("golden", "tiny") for b in (False, True)]


# ------------------------------------------------------------------------------------------------ 1. equal to the reference
@pytest.mark.parametrize("measure,shape,boolean", GRID)
def test_equal_to_the_reference(ctx, rm_golden, measure, shape, boolean):
    c = grid_case(ctx, rm_golden, measure, shape, boolean)
    assert sum(len(x or []) > 3 for x in c["allc"]) > 50                                     # how_many 1 and 3 cut real lists
    for h in HOW_MANY:
        check_against_reference(c["calls"][h], c["allc"], h, c["gu"], c["gi"])


# ------------------------------------------------------------------------------------------------ 2. bitwise the estimates
@pytest.mark.parametrize("measure,shape,boolean", GRID)
def test_bitwise_the_estimates(ctx, rm_golden, measure, shape, boolean):
    c = grid_case(ctx, rm_golden, measure, shape, boolean)
    status = [r[3] for r in c["est"]]
    assert 0 in status and 3 in status and 4 in status
    for h in HOW_MANY:
        bec = c["calls"][h]
        assert pair_bits(bec) == c["est"]
        st, es = bec.because_stats, c["est_stats"]
        for k in ("pairs_asked", "pair_offset", "by_status", "users_known", "targets"):
            assert st[k] == es[k], k
        assert bec.stats["users_scored"] == c["users_scored"]
    # the rows of a pair that is no OK pair are listed all the same
    p = c["calls"][64].pairs()
    for code in (3,) if boolean else (3, 4):                                                 # (boolean data: TOO_FEW = no contributor at all)
        assert (np.diff(p["start"])[p["status"] == code] > 0).any(), code


def test_awkward_pairs_are_answered_in_place(ctx, rm_golden):
    u, i, s = dataset("golden", rm_golden)
    o = SHAPES["golden"]
    prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"])
    known_items = np.unique(i)
    pairs = [(3, int(x)) for x in known_items[:40]] + [(3, 13), (3, 0), (3, 101), (3, -5), (3, 2 ** 31 - 1), (3, -2 ** 31)]
    pairs += [(7, 1), (31, 1), (0, 1), (-4, 1), (2 ** 31 - 1, 1), (-2 ** 31, 1), (7, 13), (-4, 13)]
    pairs += [(3, int(known_items[5]))] * 3                                                  # duplicates
    pairs += [(x, int(y)) for x in (1, 2, 5, 30) for y in known_items[::9]]
    order = np.random.default_rng(2).permutation(len(pairs))                                 # one user's pairs scattered through the input
    pu = np.array([pairs[k][0] for k in order], dtype=np.int64).astype(np.int32)
    pi = np.array([pairs[k][1] for k in order], dtype=np.int64).astype(np.int32)
    allc = BR.contributors(u, i, s, *job_sims(prepared, i), pu, pi, o["max_prefs"])
    est = prepared.estimate((pu, pi), maxPrefsPerUser=o["max_prefs"])
    bec = prepared.because((pu, pi), howMany=4, maxPrefsPerUser=o["max_prefs"])
    check_against_reference(bec, allc, 4, pu, pi)
    assert pair_bits(bec) == est_bits(est.rows())
    p = bec.pairs()
    unknown = np.isin(p["status"], (1, 2))
    assert unknown.sum() == 14 and (np.diff(p["start"])[unknown] == 0).all() and (p["contributors"][unknown] == 0).all()
    assert all((c is None) == bool(k) for c, k in zip(allc, unknown.tolist()))
    dup = np.flatnonzero((pu == 3) & (pi == known_items[5]))
    assert len(dup) == 4
    per_pair = [row_bits(bec)[p["start"][t]:p["start"][t + 1]] for t in dup]
    assert all([r[1:] for r in x] == [r[1:] for r in per_pair[0]] for x in per_pair)      # a pair asked twice is answered twice
    assert bec.because_stats["targets"] == est.estimate_stats["targets"] < len(pairs) - 14
    # a device request gives the same answer
    import torch
    dev = prepared.because((torch.from_numpy(pu).cuda(), torch.from_numpy(pi).cuda()), howMany=4, maxPrefsPerUser=o["max_prefs"])
    assert everything(dev) == everything(bec)
    prepared.close()


# ------------------------------------------------------------------------------------------------ 3. the terms are the estimate
@pytest.mark.parametrize("measure,shape,boolean", GRID)
def test_the_terms_are_the_estimate(ctx, rm_golden, measure, shape, boolean):
    c = grid_case(ctx, rm_golden, measure, shape, boolean)
    u, i, s = c["data"]
    bec = c["calls"][64]
    p, r = bec.pairs(), bec.rows()
    position = {x: {j: k for k, (j, _) in enumerate(prefs)} for x, prefs in ER.kept_preferences(u, i, s, c["o"]["max_prefs"]).items()}
    folded = 0
    for t in np.flatnonzero((p["status"] == 0) & (p["contributors"] <= 64)).tolist():
        a, b = int(p["start"][t]), int(p["start"][t + 1])
        assert b - a == p["contributors"][t]
        order = sorted(range(a, b), key=lambda k: position[int(p["user"][t])][int(r["because"][k])])      # back into preference order
        got = BR.fold([(float(r["sim"][k]), float(r["pref"][k])) for k in order], boolean)
        assert got.view(np.uint32) == p["estimate"][t:t + 1].view(np.uint32)[0], (t, got, p["estimate"][t])
        folded += 1
    assert folded >= 100


# ------------------------------------------------------------------------------------------------ 4. the block shape
def test_block_shape(ctx):
    u, i, s = BR.block_data()
    prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=100)
    si, so, sv = job_sims(prepared, i)
    assert len(si) == 80 * 79                                                                # every row holds every other item
    X, (a, b) = BR.BLOCK_X, BR.BLOCK_TWINS
    pu, pi = np.full(5, X, dtype=np.int32), np.array(BR.BLOCK_LACKS, dtype=np.int32)
    allc = BR.contributors(u, i, s, si, so, sv, pu, pi, 10)
    assert [len(c) for c in allc] == [75] * 5                                                # more than lanes, more than how_many
    tie_listed = 0
    for c in allc:
        best = sorted(c, key=BR.order_key)
        k = [e[0] for e in best].index(a)
        assert best[k + 1][0] == b and best[k][3] == best[k + 1][3]                          # equal weights, different ids
        tie_listed += k + 1 < 64
    assert tie_listed > 0
    for h in (64, 1, 7):
        bec = prepared.because((pu, pi), howMany=h, maxPrefsPerUser=10)
        check_against_reference(bec, allc, h, pu, pi)
        p = bec.pairs()
        assert p["contributors"].tolist() == [75] * 5 and np.diff(p["start"]).tolist() == [h] * 5
        if h == 64:
            for t in range(5):
                got = bec.rows()["because"][p["start"][t]:p["start"][t + 1]].tolist()
                if a in got[:-1]:
                    assert got[got.index(a) + 1] == b                                        # the tie is broken by ascending id
    est = prepared.estimate((pu, pi), maxPrefsPerUser=10)
    assert pair_bits(bec) == est_bits(est.rows()) and set(bec.pairs()["status"].tolist()) == {0}
    # the whole grid of the block: every target with 74 or 75 contributors
    gu, gi = grid_of(np.unique(u)[::7], np.unique(i))
    bec = prepared.because((gu, gi), howMany=64, maxPrefsPerUser=100)
    check_against_reference(bec, BR.contributors(u, i, s, si, so, sv, gu, gi, 100), 64, gu, gi)
    assert pair_bits(bec) == est_bits(prepared.estimate((gu, gi), maxPrefsPerUser=100).rows())
    prepared.close()


# ------------------------------------------------------------------------------------------------ 5. rows longer than a wave
def test_rows_longer_than_a_wave(ctx):
    u, i, s = dataset("ml100k", None)
    o = SHAPES["ml100k"]
    assert o["K"] > 64
    prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.COSINE)
    users = np.unique(u)[::19][:50]
    rec = prepared.recommend(users, numRecommendations=o["N"], maxPrefsPerUser=o["max_prefs"]).rows()
    pu, pi = rec["user"].copy(), rec["item"].copy()
    assert len(pu) == 50 * o["N"]
    si, so, sv = job_sims(prepared, i)
    allc = BR.contributors(u, i, s, si, so, sv, pu, pi, o["max_prefs"])
    for h in (5, 64):
        bec = prepared.because((pu, pi), howMany=h, maxPrefsPerUser=o["max_prefs"])
        check_against_reference(bec, allc, h, pu, pi)
    p, r = bec.pairs(), bec.rows()
    assert p["estimate"].view(np.uint32).tolist() == rec["score"].view(np.uint32).tolist() and (p["status"] == 0).all()
    # a listed term was found behind the 64th entry of its row
    first = {}
    for k, j in enumerate(si.tolist()):
        first.setdefault(j, k)
    at = {(j, x): k - first[j] for k, (j, x) in enumerate(zip(si.tolist(), so.tolist()))}
    assert max(at[(j, x)] for j, x in zip(r["because"].tolist(), r["item"].tolist())) >= 64
    assert bec.because_stats["row_entries_walked"] > 0 and p["contributors"].max() > 5
    prepared.close()


# ------------------------------------------------------------------------------------------------ 6. the store
def test_the_row_store_changes_nothing(ctx):
    P = pkg()
    u, i, s = dataset("tiny", None)
    o = SHAPES["tiny"]
    users = np.unique(u)[5:40]
    gu, gi = grid_of(users, np.unique(i)[::3])
    kw = dict(maxPrefsPerUser=o["max_prefs"])
    job = P.BaselineRecommenderJob(ctx)
    prepared = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.LOGLIKELIHOOD)
    cold = prepared.because((gu, gi), **kw)
    st = cold.because_stats
    assert st["rows_built"] == st["items_needed"] == st["rows_stored"] > 0 and st["rows_from_store"] == 0 and st["batches"] >= 1
    assert st["pair_contribs"] == cold.stats["pair_contribs"] > 0
    want = everything(cold)
    assert cold.size > 100 and any(r[3] == 0 for r in want[1])
    warm = prepared.because((gu, gi), **kw)
    q = warm.because_stats
    assert q["rows_built"] == 0 and q["pair_contribs"] == 0 and q["batches"] == 0 and q["rows_from_store"] == st["items_needed"]
    assert everything(warm) == want
    assert everything(prepared.because((gu, gi), **kw)) == want                              # two runs are bit-identical
    # a later recommend and a later estimate find every row of these users in the store
    rec = prepared.recommend(users, numRecommendations=o["N"], **kw)
    assert rec.request_stats["rows_built"] == 0 and rec.request_stats["rows_from_store"] == st["items_needed"] and rec.size > 0
    est = prepared.estimate((gu, gi), **kw)
    assert est.estimate_stats["rows_built"] == 0 and est.estimate_stats["rows_from_store"] == st["items_needed"]
    assert est_bits(est.rows()) == want[1]
    prepared.drop_rows()
    again = prepared.because((gu, gi), **kw)
    assert again.because_stats["rows_built"] == st["items_needed"] and everything(again) == want
    prepared.close()
    # a store filled by recommend, and one filled by estimate, for the same users
    for fill in ("recommend", "estimate"):
        fresh = job.prepare((u, i, s), maxSimilaritiesPerItem=o["K"], similarityClassname=MR.LOGLIKELIHOOD)
        if fill == "recommend":
            built = fresh.recommend(users, numRecommendations=o["N"], **kw).request_stats["rows_built"]
        else:
            built = fresh.estimate((gu, gi), **kw).estimate_stats["rows_built"]
        assert built == st["items_needed"]
        served = fresh.because((gu, gi), **kw)
        assert served.because_stats["rows_from_store"] == st["items_needed"] > 0 and served.because_stats["rows_built"] == 0
        assert everything(served) == want
        fresh.close()


# ------------------------------------------------------------------------------------------------ 7. ranks
def test_ranks_cut_the_pair_list(ctx):
    u, i, s = dataset("tiny", None)
    o = SHAPES["tiny"]
    prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=o["K"])
    gu, gi = grid_of(np.unique(u)[::5], np.unique(i)[::2])
    perm = np.random.default_rng(4).permutation(len(gu))
    gu, gi = gu[perm], gi[perm]
    kw = dict(howMany=3, maxPrefsPerUser=o["max_prefs"])
    whole = prepared.because((gu, gi), **kw)
    parts = [prepared.because((gu, gi), rank=r, world=3, **kw) for r in range(3)]
    n = len(gu)
    assert [p.because_stats["pair_offset"] for p in parts] == [n * r // 3 for r in range(3)]
    assert [p.because_stats["pairs_asked"] for p in parts] == [n * (r + 1) // 3 - n * r // 3 for r in range(3)]
    assert sum(p.size for p in parts) == whole.size > 100
    rows = [(t + p.because_stats["pair_offset"], *rest) for p in parts for (t, *rest) in row_bits(p)]
    assert rows == row_bits(whole)
    assert [x for p in parts for x in pair_bits(p)] == pair_bits(whole)
    assert [x for p in parts for x in p.pairs()["contributors"].tolist()] == whole.pairs()["contributors"].tolist()
    assert all(p.pairs()["start"][0] == 0 and p.pairs()["start"][-1] == p.size for p in parts)
    with pytest.raises(RuntimeError, match=r"BaselineRecommenderJob failed!.*rank"):
        prepared.because((gu, gi), rank=3, world=3)
    prepared.close()


# ------------------------------------------------------------------------------------------------ 8. refusals, nothing asked, NaN
def test_refusals(ctx, rm_golden):
    P = pkg()
    N = P._native
    u, i, s = dataset("golden", rm_golden)
    prepared = P.BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=20)
    for bad in (0, 65, -1):
        with pytest.raises(RuntimeError, match="howMany") as e:
            prepared.because(([1, 2], [3, 4]), howMany=bad)
        assert e.value.__cause__.code == -1               # FY_ERR_INVALID_ARGUMENT
    with pytest.raises(RuntimeError, match="maxPrefsPerUser") as e:
        prepared.because(([1, 2], [3, 4]), maxPrefsPerUser=0)
    assert e.value.__cause__.code == -1
    with pytest.raises(ValueError):
        prepared.because(([2 ** 31], [1]))
    for bad, what in ((dict(world=2), "world"), (dict(minPrefsPerUser=2), "minPrefsPerUser")):
        other = P.RowSimilarityJob(ctx).prepare((u, i, s), maxSimilaritiesPerRow=20, **bad)
        with pytest.raises(RuntimeError, match=r"BaselineRecommenderJob failed!.*" + what) as e:
            other.because(([1, 2], [3, 4]))
        assert e.value.__cause__.code == -10              # FY_ERR_UNSUPPORTED
        other.close()
    # the new kind is no list, no estimates and no similarity result; a list result has no view
    bec = prepared.because(([1, 2, 3], [3, 4, 5]), maxPrefsPerUser=8)
    test = P.Ratings(ctx, u[:50], i[:50], s[:50])
    ev = P.Evaluator(ctx, test, cutoffs=(5,), relevance_threshold=4.0)
    with pytest.raises(P.FilmYouError) as e:
        ev.evaluate(bec)
    assert e.value.code == -1
    ev.close()
    lib = N.load()
    assert lib.fy_eval_estimates(ctx._h, bec._h, test._h, None, C.byref(N.EvalErrors())) == -1
    assert lib.fy_result_itemcf_estimate_stats(bec._h, C.byref(N.ItemCFEstimateStats())) == -9
    with pytest.raises(RuntimeError) as e:
        P.BaselineRecommenderJob(ctx).run(test, similarities=bec)
    assert e.value.__cause__.code == -1
    out = C.c_void_p()
    assert lib.fy_itemsim_pairs(ctx._h, bec._h, C.byref(out)) == -1 and not out.value
    rec = prepared.recommend([1, 2, 3], numRecommendations=5)
    est = prepared.estimate(([1, 2], [3, 4]))
    for other in (rec, est):
        assert lib.fy_result_because_view(other._h, C.byref(N.ItemCFBecauseView())) == -9          # FY_ERR_STATE
        assert lib.fy_result_itemcf_because_stats(other._h, C.byref(N.ItemCFBecauseStats())) == -9
    test.close()
    # nothing asked; nobody known; a job over no preferences
    empty = np.zeros(0, dtype=np.int32)
    none = prepared.because((empty, empty))
    assert none.size == 0 and len(none.rows()["pair"]) == 0 and len(none.pairs()["user"]) == 0 and none.pairs()["start"].tolist() == [0]
    assert none.because_stats["by_status"] == [0] * 8 and none.because_stats["rows_built"] == 0
    unknown = prepared.because(([7, -1], [1, 13]))
    assert unknown.pairs()["status"].tolist() == [1, 1] and unknown.size == 0 and unknown.pairs()["start"].tolist() == [0, 0, 0]
    assert unknown.because_stats["users_known"] == 0 and unknown.because_stats["rows_built"] == 0
    prepared.close()
    z = np.zeros(0, dtype=np.int32)
    nothing = P.BaselineRecommenderJob(ctx).prepare((z, z, np.zeros(0, dtype=np.float32)))
    got = nothing.because(([1, 2], [3, 4]))
    assert got.pairs()["status"].tolist() == [1, 1] and got.size == 0
    nothing.close()


def test_a_nan_score_never_becomes_a_term(ctx):
    """Ratings accepts a NaN score, but the job's preparation drops it (as for every job of the package), so no NaN preference reaches
    the kernel: the answer is the reference's on the ratings without that entry, and the estimates'.  The NaN-last rule itself is
    held by tests/test_because_cpu.py on the statement."""
    nan = np.float32("nan")
    u = np.array([1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3], dtype=np.int32)
    i = np.array([1, 2, 3, 1, 2, 3, 4, 1, 2, 3, 4], dtype=np.int32)
    s = np.array([2.0, nan, 4.0, 3.0, 3.0, 3.0, 3.0, 5.0, 1.0, 2.0, 4.0], dtype=np.float32)
    prepared = pkg().BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=20, similarityClassname=MR.COOCCURRENCE)
    pu, pi = np.array([1, 1, 2], dtype=np.int32), np.array([4, 3, 4], dtype=np.int32)
    kept = ~np.isnan(s)
    allc = BR.contributors(u[kept], i[kept], s[kept], *job_sims(prepared, i), pu, pi, 50)
    assert [len(c) for c in allc] == [2, 1, 3]
    for h in (64, 1):
        bec = prepared.because((pu, pi), howMany=h)
        check_against_reference(bec, allc, h, pu, pi)
    assert not np.isnan(bec.rows()["pref"]).any() and pair_bits(bec) == est_bits(prepared.estimate((pu, pi)).rows())
    prepared.close()
