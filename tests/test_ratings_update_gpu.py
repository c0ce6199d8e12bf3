"""Ratings that take writes (fy_ratings_apply / Ratings.updated) on the GPU: exact equality -- order, bits and every counter -- with
the plain statement of the contract in tests/ratings_update_ref.py; both table paths; a device-resident batch; the reference's own
RM2 fixture damaged and restored by a batch; item-based CF on non-positive scores; the source left intact; an injected allocation
failure."""
import functools

import numpy as np
import pytest

from ratings_update_ref import COUNTERS, apply_writes, same_bits
from util import RTOL, pkg, synth

pytestmark = pytest.mark.gpu

BIG = 2 ** 31 - 1
ALIAS = (1 << 18) + 1            # shares its bit of the user bitmap with user 1: the bitmap says "maybe", the key search says no
USER_POOL = np.array(list(range(0, 300)) + [ALIAS, -7, BIG], dtype=np.int64)
ITEM_POOL = np.array(list(range(0, 500)) + [-3, BIG], dtype=np.int64)


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def source(n):
    """n entries over distinct keys drawn from the pools (ids 0, 1, 2^31 - 1 as user and as item, a negative id, a user that aliases
    in the bitmap), in random order, a NaN and non-positive scores among them; from 255 entries on, six of them repeat an earlier
    key (old duplicates)."""
    rng = np.random.default_rng(1000 + n)
    cells = rng.choice(len(USER_POOL) * len(ITEM_POOL), size=n, replace=False)
    u, i = USER_POOL[cells // len(ITEM_POOL)], ITEM_POOL[cells % len(ITEM_POOL)]
    s = (rng.integers(-4, 11, size=n) / 2).astype(np.float32)
    if n >= 255:
        u[0], i[0] = 0, BIG                  # the first and the last entry carry the extreme ids
        u[n - 1], i[n - 1] = BIG, 0
        for k, at in enumerate(1 + rng.choice(n // 2, size=6, replace=False)):
            u[n - 2 - 3 * k], i[n - 2 - 3 * k] = u[at], i[at]
        s[n // 3] = np.nan
    return u.astype(np.int32), i.astype(np.int32), s


def batch(src, nb, seed=0):
    """nb writes: runs of one to four writes per key with every pattern of deletes inside a run, over keys of the source (its first
    and last entry among them), of its duplicates, and new ones; shuffled."""
    su, si, _ = src
    rng = np.random.default_rng(77 + 13 * nb + len(su) + seed)
    keys = []
    if len(su):
        keys += [(int(su[-1]), int(si[-1]))]
        if nb > 1:
            keys += [(int(su[0]), int(si[0]))]
        if len(su) >= 255 and nb > 2:
            keys += [(int(su[-2]), int(si[-2]))]                       # a key the source holds twice
    while len(keys) < nb:
        if len(su) and rng.random() < 0.5:
            at = int(rng.integers(len(su)))
            keys.append((int(su[at]), int(si[at])))
        else:
            keys.append((int(rng.choice(USER_POOL)), int(rng.choice(ITEM_POOL))))
    keys = list(dict.fromkeys(keys))
    writes, pattern = [], 0
    for k, key in enumerate(keys):
        run = 1 + k % 4
        for p in range(run):
            writes.append((key[0], key[1], float(rng.integers(-4, 11)) / 2, (pattern >> p) & 1))
        pattern += k % 4 == 3                                          # every run length sees every pattern of deletes in turn
    writes = writes[:nb]
    order = rng.permutation(len(writes))
    w = [writes[k] for k in order]
    u = np.array([x[0] for x in w], dtype=np.int32)
    i = np.array([x[1] for x in w], dtype=np.int32)
    s = np.array([x[2] for x in w], dtype=np.float32)
    r = np.array([x[3] for x in w], dtype=np.uint8)
    if len(s) > 3:
        s[3] = np.nan
    return u, i, s, r


def assert_equals_reference(got, stats, src, b):
    eu, ei, es, ec = apply_writes(*src, *b)
    print({k: stats[k] for k in COUNTERS})
    assert stats == ec
    assert np.array_equal(got[0], eu) and np.array_equal(got[1], ei) and same_bits(got[2], es)


@pytest.mark.parametrize("nb", [0, 1, 7, 5000])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70001])
def test_exact_equality_with_the_reference(ctx, n, nb):
    P = pkg()
    src = source(n)
    b = batch(src, nb)
    assert len(b[0]) == nb
    R = P.Ratings(ctx, *src)
    U = R.updated(*b)
    assert U.nnz == U.update_stats["nnz_out"] and U._h.value != R._h.value
    assert_equals_reference(U.to_host(), U.update_stats, src, b)
    if nb == 5000 and n >= 255:     # the case is what it claims to be
        st = U.update_stats
        assert st["n_superseded"] > 0 and st["n_replaced"] > 0 and st["n_inserted"] > 0 and st["n_deleted"] > 0 and st["n_delete_missed"] >= 0
        assert st["n_source_dropped"] > st["n_replaced"] + st["n_deleted"]          # a duplicate of the source was cured
    if nb == 5000:
        assert U.update_stats["n_delete_missed"] > 0 and U.update_stats["n_superseded"] > 0
    # no deletes at all: remove=None
    V = R.updated(b[0], b[1], b[2])
    eu, ei, es, ec = apply_writes(*src, b[0], b[1], b[2])
    got = V.to_host()
    assert V.update_stats == ec and np.array_equal(got[0], eu) and np.array_equal(got[1], ei) and same_bits(got[2], es)
    for x in (U, V, R):
        x.close()


def test_table_in_global_memory_and_in_lds(ctx, monkeypatch):
    P = pkg()
    src = source(70001)
    b = batch(src, 5000)
    R = P.Ratings(ctx, *src)
    monkeypatch.setenv("FY_UPD_LDS_KEYS", "64")          # below the batch's distinct keys: searched in global memory
    G = R.updated(*b)
    G2 = R.updated(*b)
    monkeypatch.delenv("FY_UPD_LDS_KEYS")                # the default: the table fits in LDS
    L = R.updated(*b)
    L2 = R.updated(*b)
    g, g2, l, l2 = G.to_host(), G2.to_host(), L.to_host(), L2.to_host()
    assert_equals_reference(g, G.update_stats, src, b)
    assert G.update_stats["n_writes"] - G.update_stats["n_superseded"] > 64
    for other, st in ((g2, G2.update_stats), (l, L.update_stats), (l2, L2.update_stats)):
        assert st == G.update_stats
        assert np.array_equal(other[0], g[0]) and np.array_equal(other[1], g[1]) and same_bits(other[2], g[2])
    for x in (G, G2, L, L2, R):
        x.close()


def test_device_resident_batch(ctx):
    import torch
    P = pkg()
    src = source(70001)
    b = batch(src, 5000, seed=5)
    R = P.Ratings(ctx, *src)
    H = R.updated(*b)
    dev = torch.device("cuda", ctx.device)
    D = R.updated(torch.from_numpy(b[0]).to(dev), torch.from_numpy(b[1]).to(dev), torch.from_numpy(b[2]).to(dev), torch.from_numpy(b[3]).to(dev))
    h, d = H.to_host(), D.to_host()
    assert_equals_reference(d, D.update_stats, src, b)
    assert D.update_stats == H.update_stats
    assert np.array_equal(h[0], d[0]) and np.array_equal(h[1], d[1]) and same_bits(h[2], d[2])
    # a source made from device tensors, an empty device batch
    R2 = P.Ratings(ctx, torch.from_numpy(src[0]).to(dev), torch.from_numpy(src[1]).to(dev), torch.from_numpy(src[2]).to(dev))
    E = R2.updated(torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev))
    e = E.to_host()
    assert np.array_equal(e[0], src[0]) and np.array_equal(e[1], src[1]) and same_bits(e[2], src[2])
    for x in (H, D, E, R2, R):
        x.close()


# ---------------------------------------------------------------- the reference's own fixture, damaged and restored
def rm2_conf(g):
    P = pkg()
    conf = P.Configuration()
    conf.setInt("numberOfRecommendations", 1000)
    conf.setFloat("lambda", 0.5)
    conf.setInt("numberOfItems", g["numberOfItems"])
    conf.setInt("numberOfClusters", g["numberOfClusters"])
    return conf


def damaged_fixture(g):
    """-> (damaged arrays, the batch that restores the fixture, the users it touches)"""
    u, i, s = g["coo"]
    n = len(u)
    rng = np.random.default_rng(5)
    dropped = np.arange(n) % 7 == 6
    changed = (np.arange(n) % 5 == 4) & ~dropped
    ds = s.copy()
    ds[changed] = np.float32(np.where(s[changed] == 2.0, 4.5, 2.0))
    assert not np.any(ds[changed] == s[changed])
    extra_u = rng.integers(1, 31, size=40).astype(np.int32)
    extra_i = (int(i.max()) + 1 + np.arange(40)).astype(np.int32)                  # items the fixture does not hold
    extra_s = (rng.integers(1, 11, size=40) / 2).astype(np.float32)
    du = np.concatenate([u[~dropped], extra_u])
    di = np.concatenate([i[~dropped], extra_i])
    dsc = np.concatenate([ds[~dropped], extra_s])
    mix = rng.permutation(len(du))
    damaged = (du[mix], di[mix], dsc[mix])
    fix = dropped | changed
    bu = np.concatenate([u[fix], extra_u])
    bi = np.concatenate([i[fix], extra_i])
    bs = np.concatenate([s[fix], np.zeros(40, dtype=np.float32)])
    br = np.concatenate([np.zeros(int(fix.sum()), dtype=np.uint8), np.ones(40, dtype=np.uint8)])
    order = rng.permutation(len(bu))
    want = {"n_writes": len(bu), "n_superseded": 0, "n_replaced": int(changed.sum()), "n_inserted": int(dropped.sum()), "n_deleted": 40,
            "n_delete_missed": 0, "n_source_dropped": int(changed.sum()) + 40, "nnz_out": n}
    return damaged, (bu[order], bi[order], bs[order], br[order]), want


def bits_of(rows):
    return [rows[k].view(np.int32).tolist() if k == "score" else rows[k].tolist() for k in ("user", "item", "score", "cluster")]


def test_damaged_fixture_restored_by_a_batch(ctx, rm_golden):
    P = pkg()
    g = rm_golden
    damaged, b, want = damaged_fixture(g)
    D = P.Ratings(ctx, *damaged)
    U = D.updated(*b)
    assert U.update_stats == want
    hu, hi, hs = U.to_host()
    fixture = sorted(zip(g["coo"][0].tolist(), g["coo"][1].tolist(), g["coo"][2].tolist()))
    assert sorted(zip(hu.tolist(), hi.tolist(), hs.tolist())) == fixture            # the fixture's triples, in another order
    kw = dict(clustering=(g["map_user"], g["map_cluster"]), clustering_count=g["clusteringCount"])
    job = P.RM2Job(rm2_conf(g), ctx)
    rec = job.run(U, **kw)
    rows = rec.rows()
    exp = np.asarray(g["recommendations"])
    assert rec.size == len(exp) == 507
    got = {(int(a), int(c)): float(v) for a, c, v in zip(rows["user"], rows["item"], rows["score"])}
    assert len(got) == 507
    worst = max(abs(got[(int(a), int(c))] - v) / abs(v) for a, c, v in exp)
    print("worst relative error against the golden triples %.3g" % worst)
    assert worst <= RTOL
    # bit for bit the job on ratings created directly from the same arrays in the same order
    direct = P.Ratings(ctx, hu, hi, hs)
    rec2 = job.run(direct, **kw)
    assert bits_of(rows) == bits_of(rec2.rows())
    # the damaged object gives something else (the test can fail)
    rec3 = job.run(D, **kw)
    assert bits_of(rows) != bits_of(rec3.rows())
    # on request, for five of the touched users
    asked = np.unique(b[0])[:5].astype(np.int32)
    pu, pd = job.prepare(U, **kw), job.prepare(direct, **kw)
    try:
        ru, rd = pu.score_users(asked), pd.score_users(asked)
        a = ru.rows()
        assert bits_of(a) == bits_of(rd.rows()) and ru.size > 0
        sel = np.isin(rows["user"], asked)
        assert ru.size == int(sel.sum()) and set(a["user"].tolist()) == set(rows["user"][sel].tolist())
        for x, y, v, c in zip(a["user"], a["item"], a["score"], a["cluster"]):
            e = got[(int(x), int(y))]
            assert abs(float(v) - e) <= RTOL * abs(e)
        assert sorted(zip(a["user"].tolist(), a["item"].tolist(), a["cluster"].tolist())) == \
            sorted(zip(rows["user"][sel].tolist(), rows["item"][sel].tolist(), rows["cluster"][sel].tolist()))
    finally:
        pu.close()
        pd.close()
    for x in (rec, rec2, rec3, U, direct, D):
        x.close()


def test_item_based_cf_keeps_non_positive_scores(ctx):
    """rule 4: a score <= 0 written by a batch is data -- ratingShift = -3 makes preferences of both signs from either object."""
    P, S = pkg(), synth()
    u, i, s, _ = S.generate("ml100k", seed_offset=3)
    u, i, s = u.numpy(), i.numpy(), (np.round(s.numpy() * 2) / 2).astype(np.float32)
    rng = np.random.default_rng(8)
    at = rng.choice(len(u), size=600, replace=False)
    bu = np.concatenate([u[at], rng.integers(1, 944, size=200).astype(np.int32)])
    bi = np.concatenate([i[at], rng.integers(1, 1683, size=200).astype(np.int32)])
    bs = (rng.integers(-2, 11, size=800) / 2).astype(np.float32)                   # zeros and negatives among them
    br = (rng.random(800) < 0.25).astype(np.uint8)
    assert (bs[br == 0] <= 0).any()
    R = P.Ratings(ctx, u, i, s)
    U = R.updated(bu, bi, bs, br)
    mu, mi, ms, mc = apply_writes(u, i, s, bu, bi, bs, br)
    assert U.update_stats == mc and mc["n_replaced"] > 0 and mc["n_deleted"] > 0 and (ms <= 0).any()
    M = P.Ratings(ctx, mu, mi, ms)
    job = P.BaselineRecommenderJob(ctx)
    kw = dict(numRecommendations=20, maxPrefsPerUser=50, maxSimilaritiesPerItem=50, ratingShift=-3.0)
    rec_u, sims_u = job.run(U, **kw)
    rec_m, sims_m = job.run(M, **kw)
    a, b = rec_u.rows(), rec_m.rows()
    assert rec_u.size > 0 and all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)
    a, b = sims_u.rows(), sims_m.rows()
    assert all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)
    for x in (rec_u, rec_m, sims_u, sims_m, U, M, R):
        x.close()


def test_source_is_intact_and_keeps_its_job_state(ctx, rm_golden):
    P = pkg()
    g = rm_golden
    damaged, b, _ = damaged_fixture(g)
    D = P.Ratings(ctx, *damaged)
    kw = dict(clustering=(g["map_user"], g["map_cluster"]))
    job = P.RM2Job(rm2_conf(g), ctx)
    first = job.run(D, **kw)
    assert first.stats["prepared_from_cache"] == 0
    before = D.to_host()
    U = D.updated(*b)
    after = D.to_host()
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(before, after))
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(before, damaged))
    second = job.run(D, **kw)
    assert second.stats["prepared_from_cache"] == 1                    # the source's kept state is still valid ...
    assert bits_of(first.rows()) == bits_of(second.rows())
    mine = job.run(U, **kw)
    assert mine.stats["prepared_from_cache"] == 0                      # ... and the new object starts with none
    assert job.run(U, **kw).stats["prepared_from_cache"] == 1
    for x in (first, second, mine, U, D):
        x.close()


def test_injected_allocation_failure(ctx, rm_golden):
    P = pkg()
    g = rm_golden
    damaged, b, want = damaged_fixture(g)
    D = P.Ratings(ctx, *damaged)
    failures, nth = 0, 1
    while True:                       # every HBM request of the call in turn: a host-side refusal, nothing on the device faults
        ctx.inject_alloc_failure(nth)
        try:
            U = D.updated(*b)
        except P.FilmYouError as e:
            assert e.code == -4 and "injected fault" in e.message
            failures += 1
            nth += 1
            assert nth < 200
            continue
        finally:
            ctx.inject_alloc_failure(0)
        break
    assert failures >= 10, failures
    assert U.update_stats == want                                       # nth beyond the call's last request: it ran to completion
    lib = P._native.load()
    import ctypes as C
    ctx.inject_alloc_failure(1)
    out = C.c_void_p(1)
    assert lib.fy_ratings_apply(ctx._h, D._h, len(b[0]), b[0].ctypes.data, b[1].ctypes.data, b[2].ctypes.data, b[3].ctypes.data, 0,
                                C.byref(out), None) == -4 and out.value is None             # no result is left
    ctx.inject_alloc_failure(0)
    rec = P.RM2Job(rm2_conf(g), ctx).run(D, clustering=(g["map_user"], g["map_cluster"]))      # the source still runs a job
    rec_u = P.RM2Job(rm2_conf(g), ctx).run(U, clustering=(g["map_user"], g["map_cluster"]))
    assert rec.size > 0 and rec_u.size == 507
    for x in (rec, rec_u, U, D):
        x.close()
