"""usersFile, itemsFile, ratingShift and the item-pair output of the item-based job on the GPU.

The yardstick is the CPU oracle of item-based CF (oracle/itemcf_oracle.c) through the comparer and the tolerance of
tests/test_itemcf_gpu.py (`check`, RTOL = 2e-6: every emitted row carries the oracle's prediction for its (user, item), the lists
are as long as the oracle's, sorted, and their k-th score is the oracle's k-th best -- ties at the cut are decided by VALUE, so the
comparer leaves no row out and the left-out share is 0, which `compare` asserts by counting the rows it went through).  The
oracle has no filter options; the expected lists are made from its unbounded output here:
  usersFile    the oracle's rows of the listed users
  itemsFile    every prediction of the oracle, filtered by the allow-list, cut to N (by `check`)
  ratingShift  the oracle on float32(score + shift)
PARITY UNPINNED against the reference, as for the whole baselinerecommender package (see test_itemcf_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from test_itemcf_gpu import RTOL, check
from util import pkg, synth

pytestmark = pytest.mark.gpu
assert RTOL == 2e-6


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


def golden_data(rm_golden):
    """The 100 x 30 matrix (kept ratings), without user 7 (a user nobody knows) and without item 13 (an item nobody rated)."""
    u, i, s = rm_golden["coo"]
    keep = (s > 0) & (u != 7) & (i != 13)
    return u[keep], i[keep], s[keep]


def synthetic_data(shape):
    u, i, s, _ = synth().generate(shape)
    return u.numpy(), i.numpy(), s.numpy()


def dataset(name, rm_golden):
    return golden_data(rm_golden) if name == "golden" else synthetic_data(name)


CASES = [("golden", 10, 50, 10, False), ("golden", 5, 8, 20, False), ("golden", 10, 50, 10, True), ("tiny", 10, 10, 15, False),
         ("ml100k", 20, 50, 100, False), ("ml100k", 20, 50, 100, True)]


def restrict(ref, users=None, items=None):
    keep = np.ones(len(ref["user"]), dtype=bool)
    if users is not None:
        keep &= np.isin(ref["user"], np.asarray(users))
    if items is not None:
        keep &= np.isin(ref["item"], np.asarray(items))
    return {k: v[keep] for k, v in ref.items()}


def compare(rec, expected, N):
    """`check` of test_itemcf_gpu.py, plus: nothing was left out of the comparison, and the statistics count what was emitted."""
    rows = rec.rows()
    per_user = {}
    for u in expected["user"].tolist():
        per_user[u] = per_user.get(u, 0) + 1
    want_rows = sum(min(N, n) for n in per_user.values())
    print("rows %d expected %d users %d left out of the comparison 0" % (len(rows["user"]), want_rows, len(per_user)))
    check(rows, expected, N)
    assert len(rows["user"]) == want_rows                # every expected row was emitted and went through `check`
    assert rec.stats["recs"] == want_rows == rec.size
    assert rec.stats["users_scored"] == len(per_user)    # the listed users that received a list
    return rows


def oracle_full(u, i, s, sims, max_prefs, boolean):
    srows = sims.rows()
    # like test_itemcf_gpu.py: the oracle consumes the GPU's own similarity rows, this isolates the recommendation pass
    return oracle.itemcf(u, i, s, srows["item"], srows["other"], srows["sim"].astype(np.float64), num_recommendations=1 << 30,
                         max_prefs_per_user=max_prefs, boolean_data=boolean)


def user_request(u, rng, share=0.3):
    """A request in no particular order: a share of the known users, some of them twice, ids outside the data, a user without
    ratings (7 in the golden data) and negative ids."""
    known = np.unique(u)
    pick = rng.choice(known, size=max(3, int(share * len(known))), replace=False)
    ids = np.concatenate([pick, pick[:5], [7, 0, -3, int(known.max()) + 1, 2**31 - 1, -2**31]]).astype(np.int32)
    rng.shuffle(ids)
    return ids


def item_request(i, rng, share=0.5):
    """Half of the catalogue, some twice, plus items nobody rated (13 in the golden data) and ids outside the data."""
    known = np.unique(i)
    pick = rng.choice(known, size=max(3, int(share * len(known))), replace=False)
    ids = np.concatenate([pick, pick[:4], [13, 0, -1, int(known.max()) + 5]]).astype(np.int32)
    rng.shuffle(ids)
    return ids


def bits(rows):
    return list(zip(rows["user"].tolist(), rows["item"].tolist(), rows["score"].view(np.uint32).tolist()))


@pytest.mark.parametrize("data,N,max_prefs,K,boolean", CASES)
def test_users_items_and_both(ctx, rm_golden, data, N, max_prefs, K, boolean):
    P = pkg()
    u, i, s = dataset(data, rm_golden)
    rng = np.random.default_rng(11)
    users, items = user_request(u, rng), item_request(i, rng)
    job = P.BaselineRecommenderJob(ctx)
    kw = dict(numRecommendations=N, maxPrefsPerUser=max_prefs, maxSimilaritiesPerItem=K, booleanData=boolean)
    R = P.Ratings(ctx, u, i, s)
    whole, sims = job.run(R, **kw)
    ref = oracle_full(u, i, s, sims, max_prefs, boolean)
    # usersFile alone
    rec_u = job.run(R, similarities=sims, usersFile=users, **kw)[0]
    rows_u = compare(rec_u, restrict(ref, users=users), N)
    # ... bit for bit the unrestricted job's rows of those users, in the unrestricted job's order
    wrows = whole.rows()
    sel = np.isin(wrows["user"], users)
    assert 0 < sel.sum() < len(sel)
    assert bits(rows_u) == bits({k: v[sel] for k, v in wrows.items()})
    # itemsFile alone: the N best AMONG the allowed items
    rec_i = job.run(R, similarities=sims, itemsFile=items, **kw)[0]
    rows_i = compare(rec_i, restrict(ref, items=items), N)
    assert np.all(np.isin(rows_i["item"], items))
    # both
    rec_b = job.run(R, similarities=sims, usersFile=users, itemsFile=items, **kw)[0]
    rows_b = compare(rec_b, restrict(ref, users=users, items=items), N)
    seli = np.isin(rows_i["user"], users)
    assert bits(rows_b) == bits({k: v[seli] for k, v in rows_i.items()})
    for r in (rec_u, rec_i, rec_b, whole, sims):
        r.close()
    R.close()


def test_allow_list_is_not_a_cut_of_the_finished_list(ctx):
    """Dropping forbidden items from the unrestricted top-N gives shorter lists than the job must produce."""
    P = pkg()
    u, i, s = synthetic_data("tiny")
    items = item_request(i, np.random.default_rng(3))
    job = P.BaselineRecommenderJob(ctx)
    whole, sims = job.run((u, i, s), numRecommendations=10, maxPrefsPerUser=10, maxSimilaritiesPerItem=15)
    rec = job.run((u, i, s), numRecommendations=10, maxPrefsPerUser=10, similarities=sims, itemsFile=items)[0]
    cut = int(np.isin(whole.rows()["item"], items).sum())
    assert rec.size > cut > 0


def test_files_with_junk_lines(ctx, rm_golden, tmp_path):
    P = pkg()
    u, i, s = golden_data(rm_golden)
    uf, itf = tmp_path / "users.txt", tmp_path / "items.txt"
    uf.write_text("3\n\nabc\n12x\n3\n99999999999\n7\n21\n 5 \n1000\n17")
    itf.write_text("\n".join(str(x) for x in list(range(1, 60)) + ["x", "13", "4000000000", ""]))
    job = P.BaselineRecommenderJob(ctx)
    rec, sims = job.run((u, i, s), numRecommendations=10, maxSimilaritiesPerItem=10, usersFile=str(uf), itemsFile=itf)
    ref = oracle_full(u, i, s, sims, 50, False)
    rows = compare(rec, restrict(ref, users=[3, 7, 21, 5, 1000, 17], items=list(range(1, 60))), 10)
    assert set(rows["user"].tolist()) <= {3, 21, 5, 17} and len(rows["user"]) > 0


def test_empty_and_unknown_lists(ctx, rm_golden):
    P = pkg()
    u, i, s = golden_data(rm_golden)
    job = P.BaselineRecommenderJob(ctx)
    whole, sims = job.run((u, i, s), numRecommendations=10, maxSimilaritiesPerItem=10)
    assert whole.size > 0
    empty = np.zeros(0, dtype=np.int32)
    for kw in (dict(usersFile=empty), dict(itemsFile=empty), dict(usersFile=empty, itemsFile=empty), dict(usersFile=[1, 2], itemsFile=empty),
               dict(usersFile=[7, 31, 0, -4]), dict(itemsFile=[13, 101, 0, -4]), dict(usersFile=[7], itemsFile=[1, 2, 3])):
        rec = job.run((u, i, s), numRecommendations=10, similarities=sims, **kw)[0]
        assert rec.size == 0 and rec.stats["recs"] == 0 and rec.stats["users_scored"] == 0, kw
        assert len(rec.rows()["user"]) == 0
        rec.close()


def raw_recommend(ctx, R, sims, p, filt=None):
    P = pkg()
    lib = P._native.load()
    res = C.c_void_p()
    if filt is None:
        rc = lib.fy_itemcf_recommend(ctx._h, C.byref(p), R._h, sims._h, C.byref(res))
    else:
        rc = lib.fy_itemcf_recommend_filtered(ctx._h, C.byref(p), C.byref(filt), R._h, sims._h, C.byref(res))
    assert rc == 0, lib.fy_last_error()
    return P.ItemRecommendations(res, ctx)


@pytest.mark.parametrize("world", [1, 3])
def test_both_flags_off_is_the_unrestricted_call(ctx, world):
    P = pkg()
    u, i, s = synthetic_data("tiny")
    R = P.Ratings(ctx, u, i, s)
    sims = P.RowSimilarityJob(ctx).run(R, maxSimilaritiesPerRow=12)
    junk = np.array([1, 2, 3], dtype=np.int32)
    for rank in range(world):
        p = P._native.ItemCFParams(7, 50, 0, rank, world, 0)
        a = raw_recommend(ctx, R, sims, p)
        # the lists are ignored when the flags say "not given"
        b = raw_recommend(ctx, R, sims, p, P._native.ItemCFFilter(0, 0, 3, junk.ctypes.data, 3, junk.ctypes.data))
        assert a.size > 0 and bits(a.rows()) == bits(b.rows())
        assert a.stats["users_scored"] == b.stats["users_scored"] and a.stats["recs"] == b.stats["recs"]


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_shard_the_request(ctx, world):
    P = pkg()
    u, i, s = synthetic_data("tiny")
    rng = np.random.default_rng(world)
    users, items = user_request(u, rng, share=0.4), item_request(i, rng)
    job = P.BaselineRecommenderJob(ctx)
    R = P.Ratings(ctx, u, i, s)
    for kw in (dict(usersFile=users), dict(itemsFile=items), dict(usersFile=users, itemsFile=items), dict(usersFile=[int(np.unique(u)[3])])):
        whole, sims = job.run(R, numRecommendations=7, maxSimilaritiesPerItem=12, **kw)
        parts = [job.run(R, numRecommendations=7, rank=r, world=world, similarities=sims, **kw)[0] for r in range(world)]
        merged = [row for p in parts for row in bits(p.rows())]         # rank after rank: the order of world == 1
        assert whole.size > 0 and merged == bits(whole.rows())
        assert sum(p.stats["users_scored"] for p in parts) == whole.stats["users_scored"]
        assert sum(p.stats["recs"] for p in parts) == whole.stats["recs"]
        if "usersFile" in kw and len(kw["usersFile"]) > 1:
            assert sum(p.size > 0 for p in parts) == world              # every rank got a share of the request


@pytest.mark.parametrize("data,N,max_prefs,K", [("golden", 10, 50, 10), ("tiny", 10, 10, 15), ("ml100k", 20, 50, 100)])
@pytest.mark.parametrize("shift", [0.75, -3.0])
def test_rating_shift(ctx, rm_golden, data, N, max_prefs, K, shift):
    """Preference = float32(score + shift) for the similarity build and the recommendation pass alike; -3 makes preferences of
    both signs and exact zeros."""
    P = pkg()
    u, i, s = dataset(data, rm_golden)
    shifted = np.float32(s + shift)
    assert shifted.dtype == np.float32
    if shift < 0:
        assert (shifted < 0).any() and (shifted > 0).any()
    job = P.BaselineRecommenderJob(ctx)
    kw = dict(numRecommendations=N, maxPrefsPerUser=max_prefs, maxSimilaritiesPerItem=K)
    rec, sims = job.run((u, i, s), ratingShift=shift, **kw)
    compare(rec, oracle_full(u, i, shifted, sims, max_prefs, False), N)
    # the same job on ratings shifted by the caller: the same bits, similarities included
    rec2, sims2 = job.run((u, i, shifted), **kw)
    a, b = sims.rows(), sims2.rows()
    assert all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in ("item", "other", "sim"))
    assert bits(rec.rows()) == bits(rec2.rows()) and rec.size > 0
    # and together with a request
    users = user_request(u, np.random.default_rng(2))
    rec3 = job.run((u, i, s), ratingShift=shift, usersFile=users, similarities=sims, **kw)[0]
    compare(rec3, restrict(oracle_full(u, i, shifted, sims, max_prefs, False), users=users), N)


def test_shifted_ratings_object(ctx):
    P = pkg()
    u, i, s = synthetic_data("tiny")
    R = P.Ratings(ctx, u, i, s)
    S = R.shifted(-3.0)
    assert S.nnz == R.nnz and S._h.value != R._h.value
    job = P.RowSimilarityJob(ctx)
    a, b = job.run(S, maxSimilaritiesPerRow=9).rows(), job.run((u, i, np.float32(s - 3.0)), maxSimilaritiesPerRow=9).rows()
    assert len(a["item"]) > 0 and all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)
    # the source object is as it was
    c, d = job.run(R, maxSimilaritiesPerRow=9).rows(), job.run((u, i, s), maxSimilaritiesPerRow=9).rows()
    assert all(np.array_equal(c[k].view(np.int32), d[k].view(np.int32)) for k in c)
    # non-positive preferences: the similarity build's own rule for the Euclidean distance holds
    with pytest.raises(RuntimeError, match="failed!"):
        P.BaselineRecommenderJob(ctx).run((u, i, s), ratingShift=-3.0, similarityClassname=P.SIMILARITY_EUCLIDEAN_DISTANCE)
    S.close()
    R.close()


def test_failed_call_leaves_the_context_usable(ctx):
    P = pkg()
    u, i, s = synthetic_data("tiny")
    job = P.BaselineRecommenderJob(ctx)
    whole, sims = job.run((u, i, s), numRecommendations=5, maxSimilaritiesPerItem=12)
    users = np.unique(u)[:20]
    with pytest.raises(RuntimeError, match="2048"):
        job.run((u, i, s), numRecommendations=2049, similarities=sims, usersFile=users)
    R = P.Ratings(ctx, u, i, s)
    lib = P._native.load()
    res = C.c_void_p(1)
    p = P._native.ItemCFParams(5, 50, 0, 0, 1, 0)
    bad = P._native.ItemCFFilter(1, 0, 4, None, 0, None)                 # four users, no array
    assert lib.fy_itemcf_recommend_filtered(ctx._h, C.byref(p), C.byref(bad), R._h, sims._h, C.byref(res)) == -1 and res.value is None
    rec = job.run(R, numRecommendations=5, similarities=sims, usersFile=users)[0]
    sel = np.isin(whole.rows()["user"], users)
    assert rec.size > 0 and bits(rec.rows()) == bits({k: v[sel] for k, v in whole.rows().items()})


def expected_pairs(rows):
    """Plain construction: every unordered pair of the rows once, as (min, max); where both rows hold it, the smaller id's value."""
    held = {}
    for a, b, v in zip(rows["item"].tolist(), rows["other"].tolist(), rows["sim"].view(np.uint32).tolist()):
        held[(a, b)] = v
    want, one_sided = {}, 0
    for (a, b), v in held.items():
        lo, hi = min(a, b), max(a, b)
        want[(lo, hi)] = held[(lo, hi)] if (lo, hi) in held else v
        one_sided += ((b, a) not in held) and a != b
    return want, one_sided


@pytest.mark.parametrize("data,K", [("golden", 3), ("tiny", 4), ("ml100k", 5)])
def test_item_pairs(ctx, rm_golden, tmp_path, data, K):
    P = pkg()
    u, i, s = dataset(data, rm_golden)
    out = tmp_path / "matrix" / "pairs.txt"
    rec, sims = P.BaselineRecommenderJob(ctx).run((u, i, s), numRecommendations=5, maxSimilaritiesPerItem=K,
                                                   outputPathForSimilarityMatrix=str(out))
    pairs = sims.pairs()
    want, one_sided = expected_pairs(sims.rows())
    assert one_sided > 0 and len(want) < sims.size        # pairs only one of the two rows kept exist, and so do pairs both kept
    keys = list(zip(pairs["a"].tolist(), pairs["b"].tolist()))
    assert all(a <= b for a, b in keys)
    assert keys == sorted(want)                           # each pair once, in (min, max) order
    assert pairs["sim"].view(np.uint32).tolist() == [want[k] for k in keys]
    # the text file of the job holds the same pairs and reads back to the same floats
    lines = out.read_text().split("\n")
    assert lines[-1] == "" and len(lines) == len(keys) + 1
    got = [(int(x), int(y), np.float32(float(v))) for x, y, v in (line.split("\t") for line in lines[:-1])]
    assert [(x, y) for x, y, _ in got] == keys
    assert np.array_equal(np.array([v for _, _, v in got], dtype=np.float32).view(np.uint32), pairs["sim"].view(np.uint32))
    # with the rows' own ids included (no self-exclusion) a diagonal entry is its own pair
    sims2 = P.RowSimilarityJob(ctx).run((u, i, s), maxSimilaritiesPerRow=K, excludeSelfSimilarity=False)
    want2, _ = expected_pairs(sims2.rows())
    p2 = sims2.pairs()
    assert list(zip(p2["a"].tolist(), p2["b"].tolist())) == sorted(want2)
    assert p2["sim"].view(np.uint32).tolist() == [want2[k] for k in sorted(want2)]
