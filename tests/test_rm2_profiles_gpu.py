"""RM2 lists for given profiles and pending writes on a prepared job (fy_rm2_score_profiles / PreparedRM2.score_profiles).

Yardstick: the plain statement tests/rm2_profile_ref.py (composition in Python, fp64 DIRECT sums over the neighbours; pinned to the
reference's golden rows by tests/test_rm2_profiles_cpu.py), compared with util.assert_topn_matches at RTOL = 1e-5, purely relative
(no atol): the tolerance tests/test_rm2_request_gpu.py holds the same fp64 path to.  Every comparison also asserts the row count,
stats["recs"], profiles_scored, the group order, the labels and the statement's counters.  One model per data set, shared.

Not covered here: the refusal of more than 2^31 - 1 profiles / entries / elements (the arrays would not fit a test).
"""
import ctypes as C

import numpy as np
import pytest

import rm2_profile_ref as RP
from util import RTOL, assert_topn_matches, pkg, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


_DATA, _MODEL = {}, {}


def dataset(name, K, rm_golden=None):
    """(user, item, score, numberOfItems, numberOfClusters, map_user, map_cluster, lambda)"""
    key = (name, K)
    if key not in _DATA:
        if name == "golden":
            g = rm_golden
            u, i, s = g["coo"]
            _DATA[key] = (u, i, s, g["numberOfItems"], g["numberOfClusters"], g["map_user"], g["map_cluster"], 0.5)
        else:
            S = synth()
            u, i, s, facts = S.generate(name)
            u, i, s = u.numpy(), i.numpy(), s.numpy()
            uu = np.unique(u)
            _DATA[key] = (u, i, s, facts["n_items"], K, uu, S.hash_clustering(uu, K), 0.1)
    return _DATA[key]


def model_of(name, K, rm_golden=None, lam=None):
    d = dataset(name, K, rm_golden)
    key = (name, K, lam)
    if key not in _MODEL:
        _MODEL[key] = RP.Model(d[0], d[1], d[2], d[7] if lam is None else lam, d[3], (d[5], d[6]))
    return _MODEL[key]


def conf_of(d, top_n, filter_users=None, lam=None, **extra):
    conf = pkg().Configuration()
    conf.setInt("numberOfRecommendations", top_n)
    conf.set("lambda", repr(float(d[7] if lam is None else lam)))
    conf.setInt("numberOfItems", d[3])
    conf.setInt("numberOfClusters", d[4])
    if filter_users is not None:
        conf.setInt("filterUsers", filter_users)
    for k, v in extra.items():
        conf.set(k, v)
    return conf


def prepare(ctx, d, conf, **kw):
    return pkg().RM2Job(conf, ctx).prepare((d[0], d[1], d[2]), clustering=(d[5], d[6]), **kw)


def as_tuples(profiles):
    return [(p[0], list(p[1]), list(p[2]), p[3] if len(p) == 4 else None) for p in profiles]


def check(rec, model, profiles, base, top_n, clusters=None, filter_users=0, rank=0, world=1):
    """the result against the statement: nothing left out.  Returns the per-profile rows {position: (items, score bits)}"""
    composed, c = RP.compose(model, as_tuples(profiles), base, clusters=clusters, filter_users=filter_users, rank=rank, world=world)
    groups, ref = RP.score(model, composed, base)
    counts = [min(top_n, len(g[2])) for g in groups]
    rows, ps = rec.rows(), rec.profile_stats
    n_rows = int(sum(counts))
    assert rec.size == len(rows["user"]) == n_rows
    assert rec.stats["recs"] == n_rows and rec.stats["users_scored"] == len(groups)
    assert ps is not None and rec.request_stats is None and ps["profiles_scored"] == len(groups)
    for k in RP.COUNTERS:
        if k != "profiles_scored":
            assert ps[k] == c[k], (k, ps[k], c[k])
    # group order and labels: rows grouped by profile in the order given
    want_labels = np.concatenate([np.full(n, g[0]) for n, g in zip(counts, groups)]) if groups else np.zeros(0)
    assert np.array_equal(rows["user"], want_labels)
    relabelled = dict(rows)
    relabelled["user"] = np.concatenate([np.full(n, k) for k, n in enumerate(counts)]).astype(np.int32) if groups else rows["user"]
    if n_rows:
        worst = assert_topn_matches(relabelled, ref, top_n, rtol=RTOL)
        print("worst relative error %.3g over %d rows of %d groups" % (worst, n_rows, len(groups)))
    # per profile position (of the whole list given): its rows, for the bitwise comparisons
    lo = len(profiles) * rank // world
    listed = [k for k, e in enumerate(composed) if e is not None and e[2] and len(e[2]) < len(model.clusters[e[1]]["items"])]
    assert len(listed) == len(groups)
    out, at = {}, 0
    bits = rows["score"].view(np.int32)
    for k, n in zip(listed, counts):
        out[lo + k] = (rows["item"][at:at + n].copy(), bits[at:at + n].copy(), rows["cluster"][at:at + n].copy())
        at += n
    return out


def same(a, b):
    return a.keys() == b.keys() and all(all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) for k in a)


def rows_by_user(rec):
    r = rec.rows()
    out = {}
    bits = r["score"].view(np.int32)
    for x in np.unique(r["user"]).tolist():
        m = r["user"] == x
        out[x] = (r["item"][m], bits[m], r["cluster"][m])
    return out


def same_result(a, b):
    ra, rb = a.rows(), b.rows()
    return all(np.array_equal(ra[k].view(np.int32) if k == "score" else ra[k], rb[k].view(np.int32) if k == "score" else rb[k])
               for k in ("user", "item", "score", "cluster"))


# ------------------------------------------------------------------------------------------------ the golden fixture

@pytest.mark.parametrize("top_n", [1000, 7])
def test_unchanged_resident_profiles_are_score_users_bit_for_bit(ctx, rm_golden, top_n):
    d = dataset("golden", 0, rm_golden)
    model = model_of("golden", 0, rm_golden)
    users = np.unique(d[0])
    order = np.random.default_rng(5).permutation(users)
    # no entries; and entries that change nothing: an own item written again, a delete of an item the row does not hold
    K = {x: model.clusters[model.cluster_of[x]] for x in users.tolist()}
    own = {x: K[x]["items"][K[x]["rated"][K[x]["row"][x]]].tolist() for x in users.tolist()}
    absent = {x: sorted(set(K[x]["items"].tolist()) - set(own[x])) for x in users.tolist()}
    plain = [(int(x), [], []) for x in order]
    noop = [(int(x), [own[int(x)][0], absent[int(x)][0]], [9.0, 1.0], [0, 1]) for x in order]
    job = prepare(ctx, d, conf_of(d, top_n))
    try:
        by_user = rows_by_user(job.score_users(users.astype(np.int32)))
        assert len(by_user) == 30
        for profiles in (plain, noop):
            rec = job.score_profiles(profiles, base="resident")
            got = check(rec, model, profiles, "resident", top_n)
            assert len(got) == 30
            for k, x in enumerate(order.tolist()):
                assert all(np.array_equal(a, b) for a, b in zip(got[k], by_user[x])), x
            assert rec.profile_stats["users_unknown"] == 0 and rec.profile_stats["clusters_touched"] == 5
            assert rec.profile_stats["removes_missed"] == (30 if profiles is noop else 0)
    finally:
        job.close()


def what_if(model, users, seed):
    """per user: 3 added cluster items, 2 deleted own items, 1 item outside the cluster's set, 1 score of 0, a superseded duplicate"""
    rng = np.random.default_rng(seed)
    profiles = []
    for x in users:
        K = model.clusters[model.cluster_of[x]]
        own = K["items"][K["rated"][K["row"][x]]]
        absent = np.setdiff1d(K["items"], own)
        add = rng.choice(absent, size=3, replace=False).tolist()
        gone = rng.choice(own, size=4, replace=False).tolist()
        outside = 1000 + int(x)
        items = [add[0], gone[0], add[1], outside, gone[2], add[0], add[2], gone[1], gone[3], gone[3]]
        scores = [4.0, 1.0, 2.5, 3.0, 0.0, 1.5, 5.0, 2.0, 0.0, 3.5]          # gone[3]: a score of 0, then written again: stays
        remove = [0, 1, 0, 0, 0, 0, 0, 1, 0, 0]
        profiles.append((int(x), items, scores, remove))
    return profiles


def test_what_if_variants_on_the_golden_fixture(ctx, rm_golden):
    d = dataset("golden", 0, rm_golden)
    model = model_of("golden", 0, rm_golden)
    users = np.unique(d[0]).tolist()
    profiles = what_if(model, users, 1) + what_if(model, users[::3], 2)          # the same label twice: two groups
    job = prepare(ctx, d, conf_of(d, 10))
    try:
        rec = job.score_profiles(profiles, base="resident")
        got = check(rec, model, profiles, "resident", 10)
        ps = rec.profile_stats
        assert len(got) == 40 and ps["entries"] == 400 and ps["entries_unknown_item"] == 40 and ps["entries_nonpositive"] == 40
        assert ps["entries_superseded"] == 80 and ps["removes_hit"] == 80 and ps["removes_missed"] == 0
        assert ps["batches"] >= ps["clusters_touched"] == 5 and ps["slab_rows"] > 0 and ps["slab_pair_contribs"] == rec.stats["pair_contribs"] > 0
        # the CSR form gives the same bits; so does every profile alone
        lens = [len(p[1]) for p in profiles]
        csr = (np.array([p[0] for p in profiles]), np.concatenate([[0], np.cumsum(lens)]), np.concatenate([p[1] for p in profiles]),
               np.concatenate([p[2] for p in profiles]), np.concatenate([p[3] for p in profiles]))
        assert same_result(rec, job.score_profiles(csr, base="resident"))
        for k in (0, 17, 33):
            alone = check(job.score_profiles([profiles[k]], base="resident"), model, [profiles[k]], "resident", 10)
            assert all(np.array_equal(a, b) for a, b in zip(alone[0], got[k]))
    finally:
        job.close()


def test_whole_profiles_in_every_cluster(ctx, rm_golden):
    d = dataset("golden", 0, rm_golden)
    model = model_of("golden", 0, rm_golden)
    rng = np.random.default_rng(3)
    profiles, clusters = [], []
    for c in sorted(model.clusters):
        items = model.clusters[c]["items"]
        for n in (1, 5, len(items) - 1, len(items)):          # (the last one covers its cluster: no list)
            pick = rng.choice(items, size=n, replace=False).tolist()
            profiles.append((900 + c, pick + [pick[0], 2000], [3.0] * n + [0.0 if n == 5 else 2.0, 1.0], [0] * (n + 2)))
            clusters.append(c)
    profiles.append((3, [], []))          # empty, with the label of a resident user: WHOLE does not look at it
    clusters.append(0)
    job = prepare(ctx, d, conf_of(d, 1000, filter_users=1000))          # filterUsers is not applied to WHOLE profiles
    try:
        rec = job.score_profiles(profiles, base="whole", clusters=clusters)
        got = check(rec, model, profiles, "whole", 1000, clusters=clusters)
        ps = rec.profile_stats
        assert ps["profiles_empty"] == 1 and ps["users_unknown"] == ps["users_filtered"] == 0 and ps["clusters_touched"] == 5
        assert len(got) == 5 * 3 + 0 and ps["entries_nonpositive"] == 5
        one = job.score_profiles(profiles[:4], base="whole", clusters=0)          # one cluster for all
        assert same(check(one, model, profiles[:4], "whole", 1000, clusters=[0] * 4), {k: got[k] for k in range(3)})
        assert job.score_profiles([(3, [], [])], base="resident").size == 0          # filtered
    finally:
        job.close()


# ------------------------------------------------------------------------------------------------ ml100k shape

def ml_profiles(model, d):
    """resident profiles: the heaviest user of every cluster plus 10 writes (more than 256 composed items: two LDS blocks), a user cut
    down to exactly 256 items, a user who loses the cluster's most rated item, and 60 light users with 5 writes each"""
    rng = np.random.default_rng(9)
    u, s = d[0], d[2]
    ids, deg = np.unique(u[s > 0], return_counts=True)
    profiles = []
    for c, K in sorted(model.clusters.items()):
        n_own = K["rated"].sum(1)
        heavy = int(K["members"][np.argmax(n_own)])
        own = K["items"][K["rated"][K["row"][heavy]]]
        assert len(own) > 256
        absent = np.setdiff1d(K["items"], own)
        profiles.append((heavy, rng.choice(absent, size=10, replace=False).tolist(), [3.0] * 10, [0] * 10))
        cut = rng.choice(own, size=len(own) - 256, replace=False).tolist()
        profiles.append((heavy, cut, [0.0] * len(cut), [1] * len(cut)))
        top = int(K["items"][0])
        rater = int(K["members"][np.flatnonzero(K["rated"][:, 0])[3]])
        profiles.append((rater, [top], [0.0], [1]))
    light = ids[deg <= 60][:60]
    for x in light.tolist():
        K = model.clusters[model.cluster_of[x]]
        own = K["items"][K["rated"][K["row"][x]]]
        absent = np.setdiff1d(K["items"], own)
        items = rng.choice(absent, size=4, replace=False).tolist() + [int(own[0])]
        profiles.append((int(x), items, [4.0, 3.0, 2.0, 1.0, 0.0], [0, 0, 0, 0, 1]))
    return profiles


@pytest.mark.parametrize("K", [1, 3])
def test_ml100k_shape_blocks_chunks_batches_order_and_ranks(ctx, monkeypatch, K):
    d = dataset("ml100k", K)
    model = model_of("ml100k", K)
    widths = [len(c["items"]) for c in model.clusters.values()]
    assert all(w % 256 != 0 and w > 3 * 256 for w in widths)
    profiles = ml_profiles(model, d)
    job = prepare(ctx, d, conf_of(d, 20))
    try:
        rec = job.score_profiles(profiles, base="resident")
        got = check(rec, model, profiles, "resident", 20)
        ps = rec.profile_stats
        assert len(got) == len(profiles) and ps["batches"] == ps["clusters_touched"] == K
        composed = RP.compose(model, as_tuples(profiles), "resident")[0]
        sizes = sorted(len(e[2]) for e in composed)
        assert 256 in sizes and sizes[-1] > 256
        # column chunks of the slab build
        monkeypatch.setenv("FY_REQ_CHUNK", "64")
        assert same(check(job.score_profiles(profiles, base="resident"), model, profiles, "resident", 20), got)
        monkeypatch.delenv("FY_REQ_CHUNK")
        # batches: the light users alone, under a slab of a quarter of their union
        light = profiles[3 * K:]
        a = job.score_profiles(light, base="resident")
        rows_needed = a.profile_stats["slab_rows"]
        cap = max(70, rows_needed // (4 * K))          # slab rows: every light profile (at most 64 items) fits, a cluster's union does not
        assert rows_needed >= 3 * cap
        ws = cap * (-(-max(widths) // 32) * 32) * 8
        small = prepare(ctx, d, conf_of(d, 20), workspace_bytes=ws)
        try:
            b = small.score_profiles(light, base="resident")
            assert a.profile_stats["batches"] == K and b.profile_stats["batches"] >= 3, (a.profile_stats, b.profile_stats)
            assert b.profile_stats["slab_bytes_peak"] <= ws
            got_light = check(b, model, light, "resident", 20)
            assert same(got_light, {k - 3 * K: v for k, v in got.items() if k >= 3 * K})
        finally:
            small.close()
        tiny = prepare(ctx, d, conf_of(d, 20), workspace_bytes=1024)
        try:
            with pytest.raises(RuntimeError, match=r"RM2 failed!.*profile 1 \(label %d\) alone" % profiles[1][0]) as e:
                tiny.score_profiles(profiles, base="resident", rank=1, world=len(profiles))
            assert e.value.__cause__.code == -4          # FY_ERR_OUT_OF_MEMORY
            assert same_result(tiny.score(), job.score())          # the job still answers
        finally:
            tiny.close()
        # a shuffled order: every profile keeps its bits
        perm = np.random.default_rng(4).permutation(len(profiles)).tolist()
        shuffled = check(job.score_profiles([profiles[k] for k in perm], base="resident"), model, [profiles[k] for k in perm], "resident", 20)
        assert same({perm[k]: v for k, v in shuffled.items()}, got)
        # three ranks' ranges, concatenated
        parts = {}
        for r in range(3):
            part = job.score_profiles(profiles, base="resident", rank=r, world=3)
            assert part.profile_stats["profiles_asked"] == len(profiles)
            parts.update(check(part, model, profiles, "resident", 20, rank=r, world=3))
        assert same(parts, got)
    finally:
        job.close()


@pytest.mark.parametrize("K", [1, 3])
def test_ml100k_shape_whole_profiles(ctx, K):
    d = dataset("ml100k", K)
    model = model_of("ml100k", K)
    rng = np.random.default_rng(12)
    profiles, clusters = [], []
    for c, Kc in sorted(model.clusters.items()):
        for n in (300, 256, 3):
            pick = rng.choice(Kc["items"], size=n, replace=False).tolist()
            profiles.append((-7, pick, [1.0] * n))
            clusters.append(c)
    job = prepare(ctx, d, conf_of(d, 50))
    try:
        rec = job.score_profiles(profiles, base="whole", clusters=clusters)
        got = check(rec, model, profiles, "whole", 50, clusters=clusters)
        assert len(got) == 3 * K and set(rec.rows()["user"].tolist()) == {-7}
        again = job.score_profiles(profiles[::-1], base="whole", clusters=clusters[::-1])
        back = check(again, model, profiles[::-1], "whole", 50, clusters=clusters[::-1])
        assert same({len(profiles) - 1 - k: v for k, v in back.items()}, got)
    finally:
        job.close()


# ------------------------------------------------------------------------------------------------ edge data

@pytest.mark.parametrize("lam", [0.5, 0.0])
def test_edge_data(ctx, lam):
    """the data of test_rm2_request_gpu.py::test_edge_data: a 1-user cluster (user 1 in cluster 1), a user who rated every item of
    its cluster, an unmapped user routed to cluster 0, scores <= 0"""
    user = np.array([1, 1, 2, 2, 3, 3, 4, 4, 4, 9], dtype=np.int32)
    item = np.array([1, 2, 2, 3, 1, 3, 1, 2, 3, 5], dtype=np.int32)
    score = np.array([5, 3, 4, 1, 2, 2, 0.5, 0, -1, 3], dtype=np.float32)
    mu, mc = np.array([1, 2, 3, 4], dtype=np.int32), np.array([1, 2, 2, 0], dtype=np.int32)
    d = (user, item, score, 5, 3, mu, mc, lam)
    model = RP.Model(user, item, score, lam, 5, (mu, mc))
    assert model.clusters[1]["members"].tolist() == [1] and sorted(model.clusters[2]["items"].tolist()) == [1, 2, 3]
    job = prepare(ctx, d, conf_of(d, 10))
    try:
        # the 1-user cluster: its user with one item deleted has no neighbour (all -inf); a WHOLE profile there has one
        rec = job.score_profiles([(1, [2], [0.0], [1])], base="resident")
        check(rec, model, [(1, [2], [0.0], [1])], "resident", 10)
        assert rec.size == 1 and np.isneginf(rec.rows()["score"]).all()
        whole = [(50, [1], [2.0]), (51, [2], [2.0])]
        rec = job.score_profiles(whole, base="whole", clusters=1)
        check(rec, model, whole, "whole", 10, clusters=[1, 1])
        assert rec.size == 2 and np.isfinite(rec.rows()["score"]).all()          # the one neighbour rated both items
        # user 2 alone rated item 2 in cluster 2: deleted, it is a candidate whose only prepared rater is the user itself
        cases = [(2, [2], [0.0], [1]), (2, [3], [0.0]), (3, [2], [1.0]), (3, [1, 2], [0.0, 1.0], [1, 0]), (2, [1], [5.0])]
        rec = job.score_profiles(cases, base="resident")
        got = check(rec, model, cases, "resident", 10)
        if lam == 0.0:
            assert np.isneginf(got[0][1].view(np.float32)[got[0][0] == 2]).all()
            assert np.isneginf(rec.rows()["score"]).any()
        # covers its cluster -> no list; empty; unknown user; the unmapped user 9 and user 4 live in cluster 0
        others = [(2, [1], [1.0]), (3, [1, 3], [0.0, 0.0]), (77, [1], [1.0]), (-3, [], []), (9, [1], [2.0]), (4, [5], [1.0]), (4, [5, 1], [1.0, 0.0])]
        rec = job.score_profiles(others, base="resident")
        got = check(rec, model, others, "resident", 10)
        ps = rec.profile_stats
        assert sorted(got) == [6] and ps["profiles_empty"] == 1 and ps["users_unknown"] == 2 and ps["profiles_scored"] == 1
        assert ps["entries"] == 8 and ps["entries_nonpositive"] == 3
    finally:
        job.close()
    job = prepare(ctx, d, conf_of(d, 10, filter_users=3))
    try:
        both = [(2, [2], [0.0]), (3, [1], [0.0])]
        rec = job.score_profiles(both, base="resident")
        got = check(rec, model, both, "resident", 10, filter_users=3)
        assert sorted(got) == [1] and rec.profile_stats["users_filtered"] == 1
    finally:
        job.close()


# ------------------------------------------------------------------------------------------------ the job stays as it was

def test_repeatable_and_the_job_is_left_as_it_was(ctx, rm_golden):
    d = dataset("golden", 0, rm_golden)
    model = model_of("golden", 0, rm_golden)
    users = np.unique(d[0])
    profiles = what_if(model, users.tolist()[:12], 6)
    job, other = prepare(ctx, d, conf_of(d, 10), cache=False), prepare(ctx, d, conf_of(d, 10), cache=False)
    try:
        first = job.score_profiles(profiles, base="resident")          # before anything else ran on the job
        full_before, named_before = job.score(), job.score_users(users.astype(np.int32))
        second = job.score_profiles(profiles, base="resident")
        full_after, named_after = job.score(), job.score_users(users.astype(np.int32))
        assert first.size > 0 and same_result(first, second)
        assert same_result(full_before, full_after) and same_result(named_before, named_after)
        assert same_result(full_before, other.score()) and same_result(named_before, other.score_users(users.astype(np.int32)))
        empty = job.score_profiles([], base="resident")
        assert empty.size == 0 and empty.stats["recs"] == 0 and empty.profile_stats["profiles_asked"] == 0
        # fy_eval_lists takes the result
        P = pkg()
        test = P.Ratings(ctx, d[0], d[1], d[2])
        ev = P.Evaluator(ctx, test, cutoffs=(5,), relevance_threshold=4.0)
        try:
            e = ev.evaluate(first)
            assert e.lists == first.profile_stats["profiles_scored"] == 12
        finally:
            ev.close()
            test.close()
    finally:
        job.close()
        other.close()


def test_a_job_over_no_ratings(ctx):
    d = (np.array([1, 2], dtype=np.int32), np.array([1, 2], dtype=np.int32), np.array([0.0, -1.0], dtype=np.float32), 5, 1,
         np.array([1, 2], dtype=np.int32), np.array([0, 0], dtype=np.int32), 0.5)
    job = prepare(ctx, d, conf_of(d, 10))
    try:
        rec = job.score_profiles([(1, [1], [1.0])], base="whole", clusters=0)
        assert rec.size == 0 and rec.profile_stats["profiles_asked"] == 1 and rec.profile_stats["profiles_scored"] == 0
    finally:
        job.close()


# ------------------------------------------------------------------------------------------------ failures

def test_failures_leave_the_job_usable(ctx, rm_golden):
    P = pkg()
    N = P._native
    lib = N.load()
    d = dataset("golden", 0, rm_golden)
    job = prepare(ctx, d, conf_of(d, 10))
    labels = np.array([3, 4], dtype=np.int32)
    start = np.array([0, 1, 2], dtype=np.int64)
    item = np.array([1, 2], dtype=np.int32)
    score = np.array([1.0, 2.0], dtype=np.float32)
    cl = np.array([0, 1], dtype=np.int32)
    ptr = lambda a: a.ctypes.data

    def call(h, n=2, user=labels, st=start, it=item, sc=score, cluster=cl, base=0, rank=0, world=1):
        q = N.RM2Profiles(n, ptr(user) if user is not None else None, ptr(st) if st is not None else None, ptr(it) if it is not None else None,
                          ptr(sc) if sc is not None else None, None, ptr(cluster) if cluster is not None else None, base, rank, world)
        out = C.c_void_p()
        rc = lib.fy_rm2_score_profiles(h, C.byref(q), C.byref(out))
        assert (rc == 0) == bool(out.value)
        if out.value:
            lib.fy_result_free(out)
        return rc

    try:
        good = job.score_profiles([(3, [1], [1.0]), (4, [2], [2.0])], base="whole", clusters=[0, 1])
        assert call(job._h) == 0
        INVALID, UNSUPPORTED = -1, -10
        assert call(job._h, user=None) == INVALID and call(job._h, st=None) == INVALID
        assert call(job._h, it=None) == INVALID and call(job._h, sc=None) == INVALID
        assert call(job._h, st=np.array([1, 1, 2], dtype=np.int64)) == INVALID
        assert call(job._h, st=np.array([0, 2, 1], dtype=np.int64)) == INVALID
        assert call(job._h, base=2) == INVALID and call(job._h, base=-1) == INVALID
        assert call(job._h, n=-1) == INVALID
        for rank, world in ((0, 0), (-1, 1), (1, 1), (2, 2), (0, -3)):
            assert call(job._h, rank=rank, world=world) == INVALID
        assert call(job._h, cluster=None) == INVALID and call(job._h, cluster=None, base=1) == 0
        assert call(job._h, cluster=np.array([0, 10], dtype=np.int32)) == INVALID          # outside [0, numberOfClusters)
        assert call(job._h, cluster=np.array([-1, 0], dtype=np.int32)) == INVALID
        assert call(job._h, cluster=np.array([0, 7], dtype=np.int32)) == INVALID           # an empty cluster
        assert b"empty cluster" in lib.fy_last_error()
        assert call(job._h, cluster=np.array([0, 7], dtype=np.int32), base=1) == 0          # ignored with ON_RESIDENT
        assert call(job._h, n=0, user=None, st=None, it=None, sc=None, cluster=None) == 0  # zero profiles
        assert same_result(good, job.score_profiles([(3, [1], [1.0]), (4, [2], [2.0])], base="whole", clusters=[0, 1]))
        # request_stats of other result kinds, and of this kind, still say FY_ERR_STATE
        full = job.score()
        assert lib.fy_result_rm2_profile_stats(full._h, C.byref(N.RM2ProfileStats())) == -9 and full.profile_stats is None
        named = job.score_users(labels)
        assert lib.fy_result_rm2_profile_stats(named._h, C.byref(N.RM2ProfileStats())) == -9 and named.profile_stats is None
        assert lib.fy_result_request_stats(good._h, C.byref(N.RM2RequestStats())) == -9 and good.request_stats is None
        assert lib.fy_result_itemcf_profile_stats(good._h, C.byref(N.ItemCFProfileStats())) == -9
        with pytest.raises(RuntimeError, match="RM2 failed!") as e:
            job.score_profiles([(3, [1], [1.0])], base="whole", clusters=[7])
        assert e.value.__cause__.code == INVALID

        # jobs that are not served
        for extra in (dict(relevanceModel="rm1"), dict(smoothing="dirichlet", mu="100"), dict(smoothing="absoluteDiscounting", delta="0.5")):
            other = prepare(ctx, d, conf_of(d, 10, **extra))
            try:
                assert call(other._h) == UNSUPPORTED
                assert other.score_users(labels).size > 0
            finally:
                other.close()
        two = P.RM2Job(conf_of(d, 10), ctx).prepare((d[0], d[1], d[2]), clustering=(d[5], d[6]), rank=0, world=2)
        try:
            assert call(two._h) == UNSUPPORTED and b"world" in lib.fy_last_error()
        finally:
            two.close()

        class Identity:      # collectives of a world of one
            def all_gather(self, send, recv, n, stream):
                raise AssertionError("not reached")

            def reduce_scatter_f32(self, send, recv, n, stream):
                raise AssertionError("not reached")

        job.set_collectives(Identity())
        assert call(job._h) == UNSUPPORTED and b"collectives" in lib.fy_last_error()
    finally:
        job.close()
