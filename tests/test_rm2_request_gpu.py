"""RM2 on request (fy_rm2_score_users / PreparedRM2.score_users): the lists of the named users against the CPU oracle.

Yardstick: oracle.rm2 with an unbounded list length (tests/test_rm2_gpu.py: oracle_full), its rows filtered to the requested
users that it lists, compared with util.assert_topn_matches at RTOL = 1e-5, purely relative (no atol): the restricted pass is
fp64, the residue is the float cast.  Every comparison also asserts the row count, stats["recs"] and users_scored.
One oracle run per (dataset, clustering, lambda), shared by the tests.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from util import RTOL, assert_topn_matches, pkg, synth

pytestmark = pytest.mark.gpu

RESTRICTED, FULL = "2", "0"      # FY_REQ_FULL_SHARE: a share no cluster exceeds / a share every touched cluster exceeds
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


_DATA, _REF = {}, {}


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


def reference(name, K, rm_golden=None):
    key = (name, K)
    if key not in _REF:
        u, i, s, n_items, Kc, mu, mc, lam = dataset(name, K, rm_golden)
        _REF[key] = oracle.rm2(u, i, s, lam=lam, number_of_items=n_items, number_of_recommendations=1 << 30, number_of_clusters=Kc,
                               map_user=mu, map_cluster=mc, n_threads=8)
    return _REF[key]


def conf_of(d, top_n, filter_users=None, lam=None):
    P = pkg()
    conf = P.Configuration()
    conf.setInt("numberOfRecommendations", top_n)
    conf.set("lambda", repr(float(d[7] if lam is None else lam)))
    conf.setInt("numberOfItems", d[3])
    conf.setInt("numberOfClusters", d[4])
    if filter_users is not None:
        conf.setInt("filterUsers", filter_users)
    return conf


def request_of(u, s, seed, extra=()):
    """about 30 % of the known users, shuffled, some listed twice, plus ids that must be passed over"""
    known = np.unique(u[s > 0])
    rng = np.random.default_rng(seed)
    pick = rng.choice(known, size=max(1, int(0.3 * len(known))), replace=False)
    twice = pick[: max(1, len(pick) // 5)]
    unrated = np.setdiff1d(np.unique(u), known)[:1]          # an id whose ratings are all dropped by score > 0 (if any)
    hole = np.setdiff1d(np.arange(1, int(u.max()) + 2), np.unique(u))[:1]      # an id without ratings
    junk = np.array([0, -5, int(u.max()) + 1, I32_MIN, I32_MAX], dtype=np.int64)
    ids = np.concatenate([pick, twice, unrated, hole, junk, np.asarray(extra, dtype=np.int64)])
    rng.shuffle(ids)
    return ids.astype(np.int32)


def expected(ref, ids, filter_users=0):
    """the oracle's rows of the requested users that it lists"""
    keep = np.isin(ref["rec_user"], np.asarray(ids)) & (ref["rec_user"] >= filter_users)
    return {k: ref[k][keep] for k in ("rec_user", "rec_item", "rec_score", "rec_cluster")}


def check(rec, exp, top_n):
    """nothing left out: rows, stats["recs"], users_scored"""
    users, counts = np.unique(exp["rec_user"], return_counts=True)
    n_rows = int(np.minimum(counts, top_n).sum())
    rows = rec.rows()
    assert rec.size == len(rows["user"]) == n_rows
    assert rec.stats["recs"] == n_rows
    assert rec.stats["users_scored"] == len(users)
    assert rec.request_stats is not None
    if n_rows == 0:
        return 0.0
    worst = assert_topn_matches(rows, exp, top_n, rtol=RTOL)
    print("worst relative error %.3g over %d rows" % (worst, n_rows))
    return worst


def prepare(ctx, d, conf, **kw):
    P = pkg()
    return P.RM2Job(conf, ctx).prepare((d[0], d[1], d[2]), clustering=(d[5], d[6]), **kw)


def device_doubles(ptr, n):
    par = __import__("importlib").import_module("filmyou-core_amd.parallel")
    return torch.as_tensor(par._DevicePointer(ptr, n, "<f8"), device="cuda:0")


def same_rows(a, b):
    ra, rb = a.rows(), b.rows()
    return all(np.array_equal(ra[k].view(np.int32) if k == "score" else ra[k], rb[k].view(np.int32) if k == "score" else rb[k])
               for k in ("user", "item", "score", "cluster"))


def heaviest_and_lightest(u, s):
    ids, n = np.unique(u[s > 0], return_counts=True)
    return [int(ids[np.argmax(n)]), int(ids[np.argmin(n)])]


CASES = [("golden", 0, 1000), ("golden", 0, 7), ("tiny", 1, 50), ("tiny", 7, 20), ("ml100k", 1, 100), ("ml100k", 20, 50)]


@pytest.mark.parametrize("name,K,top_n", CASES)
def test_request_matches_oracle(ctx, rm_golden, monkeypatch, name, K, top_n):
    monkeypatch.setenv("FY_REQ_FULL_SHARE", RESTRICTED)
    d = dataset(name, K, rm_golden)
    ref = reference(name, K, rm_golden)
    extra = heaviest_and_lightest(d[0], d[2]) if name == "ml100k" else ()
    ids = request_of(d[0], d[2], 11, extra)
    job = prepare(ctx, d, conf_of(d, top_n))
    try:
        rec = job.score_users(ids)
        check(rec, expected(ref, ids), top_n)
        rq = rec.request_stats
        assert rq["users_asked"] == len(ids) and rq["full_pass_clusters"] == 0 and rq["batches"] >= rq["clusters_touched"] >= 1
        assert rq["users_known"] == len(np.intersect1d(ids, np.unique(d[0][d[2] > 0])))
        # users in the order of the unrestricted job
        full = job.score()
        fu = full.rows()["user"]
        order = fu[np.r_[True, fu[1:] != fu[:-1]]]
        ru = rec.rows()["user"]
        mine = ru[np.r_[True, ru[1:] != ru[:-1]]]
        assert np.array_equal(mine, order[np.isin(order, mine)])
        # one user
        one = job.score_users(ids[:0].tolist() + [int(np.unique(d[0][d[2] > 0])[3])])
        check(one, expected(ref, [int(np.unique(d[0][d[2] > 0])[3])]), top_n)
        assert one.request_stats["clusters_touched"] == 1
    finally:
        job.close()


@pytest.mark.parametrize("side", [RESTRICTED, FULL])
@pytest.mark.parametrize("name,K,top_n", [("golden", 0, 1000), ("tiny", 7, 20), ("ml100k", 20, 50)])
def test_all_users_through_either_path(ctx, rm_golden, monkeypatch, name, K, top_n, side):
    monkeypatch.setenv("FY_REQ_FULL_SHARE", side)
    d = dataset(name, K, rm_golden)
    ref = reference(name, K, rm_golden)
    ids = np.unique(d[0]).astype(np.int32)
    job = prepare(ctx, d, conf_of(d, top_n))
    try:
        rec = job.score_users(ids)
        check(rec, expected(ref, ids), top_n)
        rq = rec.request_stats
        assert rq["full_pass_clusters"] == (rq["clusters_touched"] if side == FULL else 0)
        assert (rq["slab_rows"] == 0) == (side == FULL)
        if side == FULL:
            assert same_rows(rec, job.score())
    finally:
        job.close()


def test_batches_under_a_small_workspace(ctx, monkeypatch):
    monkeypatch.setenv("FY_REQ_FULL_SHARE", RESTRICTED)
    d = dataset("ml100k", 1)
    ref = reference("ml100k", 1)
    # 200 light users (at most 100 ratings each): their union is far larger than any one of them, so a slab of a quarter of the
    # union holds every single user and forces at least four batches
    known, deg = np.unique(d[0][d[2] > 0], return_counts=True)
    ids = known[deg <= 100][:200].astype(np.int32)
    whole = prepare(ctx, d, conf_of(d, 100))
    n_items_c = len(np.unique(d[1][d[2] > 0]))
    a = whole.score_users(ids)
    rows_needed = a.request_stats["slab_rows"]
    assert rows_needed // 4 >= 100
    ws = (rows_needed // 4) * (-(-n_items_c // 32) * 32) * 8
    small = prepare(ctx, d, conf_of(d, 100), workspace_bytes=ws)
    try:
        b = small.score_users(ids)
        assert a.request_stats["batches"] == 1 and b.request_stats["batches"] >= 3, (a.request_stats, b.request_stats)
        assert b.request_stats["slab_bytes_peak"] <= ws
        assert same_rows(a, b)
        check(b, expected(ref, ids), 100)
        # a user whose own rows do not fit
        tiny = prepare(ctx, d, conf_of(d, 100), workspace_bytes=1024)
        with pytest.raises(RuntimeError, match=r"RM2 failed!.*user \d+ alone"):
            tiny.score_users(ids)
        tiny.close()
    finally:
        whole.close()
        small.close()


@pytest.mark.parametrize("lam", [0.5, 0.0])
@pytest.mark.parametrize("side", [RESTRICTED, FULL])
def test_edge_data(ctx, monkeypatch, lam, side):
    """the data of test_rm2_gpu.py::test_edge_cases_match_oracle: a 1-user cluster, a user who rated every item of its cluster, an
    unmapped user routed to cluster 0, scores <= 0; at lambda = 0 the -inf scores are kept"""
    monkeypatch.setenv("FY_REQ_FULL_SHARE", side)
    user = np.array([1, 1, 2, 2, 3, 3, 4, 4, 4, 9], dtype=np.int32)
    item = np.array([1, 2, 2, 3, 1, 3, 1, 2, 3, 5], dtype=np.int32)
    score = np.array([5, 3, 4, 1, 2, 2, 0.5, 0, -1, 3], dtype=np.float32)
    mu, mc = np.array([1, 2, 3, 4], dtype=np.int32), np.array([1, 2, 2, 0], dtype=np.int32)
    d = (user, item, score, 5, 3, mu, mc, lam)
    ref = oracle.rm2(user, item, score, lam=lam, number_of_items=5, number_of_recommendations=1 << 30, number_of_clusters=3,
                     map_user=mu, map_cluster=mc, n_threads=1)
    job = prepare(ctx, d, conf_of(d, 10))
    try:
        for ids in ([1, 2, 3, 4, 9], [9, 4], [2], [1], [3, 3, 7, -1, 0]):
            rec = job.score_users(np.array(ids, dtype=np.int32))
            check(rec, expected(ref, ids), 10)
        if lam == 0.0:
            assert np.isneginf(job.score_users(np.array([1, 2, 3, 4, 9], dtype=np.int32)).rows()["score"]).any()
    finally:
        job.close()


def test_filter_users(ctx, rm_golden, monkeypatch):
    monkeypatch.setenv("FY_REQ_FULL_SHARE", RESTRICTED)
    d = dataset("golden", 0, rm_golden)
    ref = reference("golden", 0, rm_golden)
    job = prepare(ctx, d, conf_of(d, 10, filter_users=12))
    try:
        ids = np.array([3, 11, 12, 13, 29], dtype=np.int32)
        rec = job.score_users(ids)
        check(rec, expected(ref, ids, filter_users=12), 10)
        assert sorted(set(rec.rows()["user"].tolist())) == [12, 13, 29]
    finally:
        job.close()


def test_work_is_sized_by_the_request(ctx, monkeypatch):
    monkeypatch.setenv("FY_REQ_FULL_SHARE", RESTRICTED)
    d = dataset("ml100k", 20)
    u, i, s = d[0], d[1], d[2]
    keep = s > 0
    u, i = u[keep], i[keep]
    cluster_of = dict(zip(d[5].tolist(), d[6].tolist()))
    cl = np.array([cluster_of[x] for x in u.tolist()])
    two = np.unique(cl)[:2]
    ids = np.concatenate([np.unique(u[cl == c])[:6] for c in two]).astype(np.int32)
    job = prepare(ctx, d, conf_of(d, 50))
    try:
        rec = job.score_users(ids)
        check(rec, expected(reference("ml100k", 20), ids), 50)
        rq = rec.request_stats
        deg = dict(zip(*np.unique(u, return_counts=True)))
        rows = contribs = 0
        for c in two:
            J = np.unique(i[np.isin(u, ids) & (cl == c)])
            rows += len(J)
            inside = (cl == c) & np.isin(i, J)          # the raters v of the rows j in J, inside the cluster: each walks its n_v entries
            contribs += int(sum(deg[v] for v in u[inside].tolist()))
        assert rq["clusters_touched"] == 2 and rq["full_pass_clusters"] == 0
        assert rq["slab_rows"] == rows
        assert rq["slab_pair_contribs"] == contribs == rec.stats["pair_contribs"]
        assert rec.stats["cooc_matrix_bytes"] > 0
        assert contribs < job.score().stats["pair_contribs"]
    finally:
        job.close()


def test_reproducible_and_repeatable(ctx, monkeypatch):
    """two identical requests give the same bits; a request, score(), the request again: the job stays valid and unchanged"""
    monkeypatch.setenv("FY_REQ_FULL_SHARE", RESTRICTED)
    d = dataset("ml100k", 20)
    ids = request_of(d[0], d[2], 3)
    job, other = prepare(ctx, d, conf_of(d, 50), cache=False), prepare(ctx, d, conf_of(d, 50), cache=False)
    try:
        a = job.score_users(ids)
        b = job.score_users(ids)
        full = job.score()
        c = job.score_users(ids)
        assert a.size > 0 and same_rows(a, b) and same_rows(a, c)
        assert same_rows(full, other.score())
        empty = job.score_users(np.zeros(0, dtype=np.int32))
        assert empty.size == 0 and empty.stats["recs"] == 0 and empty.request_stats["users_asked"] == 0
        assert job.score_users(np.array([-1, 0, I32_MAX], dtype=np.int32)).size == 0
    finally:
        job.close()
        other.close()


def test_errors(ctx, rm_golden):
    P = pkg()
    d = dataset("golden", 0, rm_golden)
    job = prepare(ctx, d, conf_of(d, 10))
    lib = P._native.load()
    try:
        out = C.c_void_p()
        rq = P._native.RM2Request(3, None)
        assert lib.fy_rm2_score_users(job._h, C.byref(rq), C.byref(out)) == -1 and not out.value
        st = P._native.RM2RequestStats()
        full = job.score()
        assert lib.fy_result_request_stats(full._h, C.byref(st)) == -9 and full.request_stats is None

        class Identity:      # collectives of a world of one
            def all_gather(self, send, recv, n, stream):
                raise AssertionError("not reached")

            def reduce_scatter_f32(self, send, recv, n, stream):
                raise AssertionError("not reached")

        job.set_collectives(Identity())
        ids = np.array([1, 2], dtype=np.int32)
        rq = P._native.RM2Request(2, ids.ctypes.data)
        assert lib.fy_rm2_score_users(job._h, C.byref(rq), C.byref(out)) == -10 and not out.value
    finally:
        job.close()


def test_two_ranks(ctx, monkeypatch):
    """world 2, replicated statistics exchanged by hand (tests/test_multirank_gpu.py: sharded_equals_single), no collectives"""
    monkeypatch.setenv("FY_REQ_FULL_SHARE", RESTRICTED)
    P = pkg()
    d = dataset("ml100k", 1)
    ref = reference("ml100k", 1)
    ids = request_of(d[0], d[2], 7)
    conf = conf_of(d, 100)
    ratings = P.Ratings(ctx, d[0], d[1], d[2])
    job = P.RM2Job(conf, ctx)
    prepared = [job.prepare(ratings, clustering=(d[5], d[6]), rank=r, world=2) for r in range(2)]
    parts = []
    for pr in prepared:
        ptr, n = pr.partial_stats()
        parts.append(device_doubles(ptr, n).clone())
    torch.cuda.synchronize()
    gathered = torch.cat(parts).contiguous()
    torch.cuda.synchronize()
    results = []
    for pr in prepared:
        pr.set_global_stats(gathered.data_ptr())
        results.append(pr.score_users(ids))
    single = prepare(ctx, d, conf)
    try:
        one = single.score_users(ids)
        rows = {k: np.concatenate([r.rows()[k] for r in results]) for k in ("user", "item", "score", "cluster")}
        owners = [set(r.rows()["user"].tolist()) for r in results]
        assert all(owners) and not (owners[0] & owners[1])
        assert owners[0] | owners[1] == set(one.rows()["user"].tolist())
        exp = expected(ref, ids)
        assert len(rows["user"]) == one.size == sum(r.stats["recs"] for r in results)
        assert sum(r.stats["users_scored"] for r in results) == len(np.unique(exp["rec_user"]))
        order = np.argsort(rows["user"], kind="stable")
        assert_topn_matches({k: v[order] for k, v in rows.items()}, exp, 100, rtol=RTOL)
        check(one, exp, 100)
    finally:
        single.close()
        for pr in prepared:
            pr.close()
        ratings.close()


@pytest.mark.parametrize("K,top_n", [(1, 100), (20, 50)])
def test_column_chunks_of_the_slab_build(ctx, monkeypatch, K, top_n):
    """FY_REQ_CHUNK = 64 and 256 cut the ml100k clusters into many column chunks (the shape of an ML-25M cluster under the default
    8192): I_c is no multiple of either, the K = 20 clusters are narrower than some chunk widths (the chunk is clamped, the offset
    table is not).  The fixed-point sums do not depend on the chunking: rows are bit-identical to the one-chunk run.  Changing the
    width on one job rebuilds the kept chunk-offset table."""
    monkeypatch.setenv("FY_REQ_FULL_SHARE", RESTRICTED)
    d = dataset("ml100k", K)
    ref = reference("ml100k", K)
    ids = request_of(d[0], d[2], 13, heaviest_and_lightest(d[0], d[2]))
    exp = expected(ref, ids)
    n_items_max = max(len(np.unique(d[1][(d[2] > 0) & np.isin(d[0], d[5][d[6] == c])])) for c in range(K))
    job = prepare(ctx, d, conf_of(d, top_n))
    try:
        one_chunk = job.score_users(ids)
        check(one_chunk, exp, top_n)
        for chunk in ("64", "256", "64"):
            assert n_items_max > int(chunk) and (K > 1 or n_items_max % int(chunk) != 0)
            monkeypatch.setenv("FY_REQ_CHUNK", chunk)
            rec = job.score_users(ids)
            check(rec, exp, top_n)
            assert same_rows(rec, one_chunk)
            assert same_rows(rec, job.score_users(ids))                  # reproducible
            assert rec.request_stats["slab_pair_contribs"] == one_chunk.request_stats["slab_pair_contribs"]
        # batches under a small slab, many chunks: light users (at most 100 ratings), a slab of 100 rows of the widest cluster
        known, deg = np.unique(d[0][d[2] > 0], return_counts=True)
        light = known[deg <= 100][:300].astype(np.int32)
        unbatched = job.score_users(light)
        small = prepare(ctx, d, conf_of(d, top_n), workspace_bytes=100 * (-(-n_items_max // 32) * 32) * 8)
        try:
            b = small.score_users(light)
            assert b.request_stats["batches"] > unbatched.request_stats["batches"] == unbatched.request_stats["clusters_touched"]
            assert same_rows(b, unbatched)
            check(b, expected(ref, light), top_n)
        finally:
            small.close()
        monkeypatch.delenv("FY_REQ_CHUNK")
        assert same_rows(job.score_users(ids), one_chunk)
    finally:
        job.close()


def test_two_ranks_with_sharded_prep(ctx, monkeypatch):
    """world 2 over 20 clusters: every rank preps its own clusters' ratings alone (statistics by raw id); the requests of the two
    ranks are disjoint and together the one-rank request"""
    monkeypatch.setenv("FY_REQ_FULL_SHARE", RESTRICTED)
    P = pkg()
    d = dataset("ml100k", 20)
    ref = reference("ml100k", 20)
    ids = request_of(d[0], d[2], 17)
    conf = conf_of(d, 50)
    ratings = P.Ratings(ctx, d[0], d[1], d[2])
    job = P.RM2Job(conf, ctx)
    prepared = [job.prepare(ratings, clustering=(d[5], d[6]), rank=r, world=2) for r in range(2)]
    single = prepare(ctx, d, conf)
    try:
        assert all(pr.stats_layout()[1] > 0 for pr in prepared)          # sharded prep
        parts = []
        for pr in prepared:
            ptr, n = pr.partial_stats()
            parts.append(device_doubles(ptr, n).clone())
        torch.cuda.synchronize()
        gathered = torch.cat(parts).contiguous()
        results = []
        for pr in prepared:
            pr.set_global_stats(gathered.data_ptr())
            results.append(pr.score_users(ids))
        one = single.score_users(ids)
        exp = expected(ref, ids)
        owners = [set(r.rows()["user"].tolist()) for r in results]
        assert all(owners) and not (owners[0] & owners[1])
        assert owners[0] | owners[1] == set(one.rows()["user"].tolist())
        assert sum(r.stats["recs"] for r in results) == one.size
        assert sum(r.stats["users_scored"] for r in results) == len(np.unique(exp["rec_user"]))
        rows = {k: np.concatenate([r.rows()[k] for r in results]) for k in ("user", "item", "score", "cluster")}
        order = np.argsort(rows["user"], kind="stable")
        assert_topn_matches({k: v[order] for k, v in rows.items()}, exp, 50, rtol=RTOL)
        check(one, exp, 50)
    finally:
        single.close()
        for pr in prepared:
            pr.close()
        ratings.close()


def test_job_run_with_a_users_file(ctx, rm_golden, tmp_path, monkeypatch):
    """RM2Job.run(usersFile=path) and run(usersFile=array): the id file is read by the library, the rows are the request's"""
    monkeypatch.setenv("FY_REQ_FULL_SHARE", RESTRICTED)
    P = pkg()
    d = dataset("golden", 0, rm_golden)
    ref = reference("golden", 0, rm_golden)
    f = tmp_path / "users.txt"
    f.write_text("17\n3\n\n3\nabc\n29\n1000\n-4")
    job = P.RM2Job(conf_of(d, 10), ctx)
    by_file = job.run((d[0], d[1], d[2]), clustering=(d[5], d[6]), usersFile=str(f))
    check(by_file, expected(ref, [3, 17, 29]), 10)
    assert by_file.request_stats["users_asked"] == 6 and by_file.request_stats["users_known"] == 3
    by_array = job.run((d[0], d[1], d[2]), clustering=(d[5], d[6]), usersFile=np.array([29, 17, 3]))
    assert same_rows(by_file, by_array)
    whole = job.run((d[0], d[1], d[2]), clustering=(d[5], d[6]))
    assert whole.request_stats is None and whole.size > by_file.size
