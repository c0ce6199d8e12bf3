"""The RM1 estimator on the GPU (relevanceModel = rm1, FY_RM2_ESTIMATOR_RM1) through every entry point of the RM2 job.

Yardstick: tests/rm1_definition.py, the dense statement (log-sum-exp over the neighbours of a dense user model), which
tests/test_rm1_cpu.py pins to a brute-force product and to the sparse form.  Criterion: util.RTOL = 1e-5, purely relative, no atol,
through util.assert_topn_matches -- every emitted row is compared, non-finite scores by equality.  The scores are never near 0
(tiny: [-1242, -42], ML-100K shape: [-7378, -75]), and every case holds rows below -745: a pass that exponentiated a likelihood
without the shift would return -inf there."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import eval_ref
from rm1_definition import definition_full
from util import RTOL, assert_topn_matches, pkg, synth

pytestmark = pytest.mark.gpu

KEY = {"jm": "lambda", "dirichlet": "mu", "absoluteDiscounting": "delta"}
HAND = (np.array([1, 1, 2, 2, 2, 3, 3, 3, 4, 5, 5], dtype=np.int32), np.array([1, 2, 1, 2, 3, 1, 2, 4, 5, 1, 5], dtype=np.int32),
        np.array([4, 2, 5, 3, 1, 2, 2, 4, 3, 1, 5], dtype=np.float32))


def conf_of(method, param, n_items, K, top_n, model="rm1", filter_users=0):
    conf = pkg().Configuration()
    conf.set("relevanceModel", model)
    conf.set("smoothing", method)
    conf.set(KEY[method], repr(float(param)))
    conf.setInt("numberOfItems", n_items)
    conf.setInt("numberOfClusters", K)
    conf.setInt("numberOfRecommendations", top_n)
    if filter_users:
        conf.setInt("filterUsers", filter_users)
    return conf


@functools.lru_cache(maxsize=None)
def shape_data(shape, K):
    S = synth()
    u, i, s, facts = S.generate(shape)
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    uu = np.unique(u)
    return (u, i, s), (uu, S.hash_clustering(uu, K)), facts["n_items"]


@functools.lru_cache(maxsize=None)
def dense_reference(shape, K, method, param):
    data, clustering, _ = shape_data(shape, K)
    return definition_full(*data, method, param, clustering=clustering)


def bits(rows):
    return {k: (rows[k].view(np.int32) if k == "score" else rows[k]) for k in ("user", "item", "score", "cluster")}


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return all(np.array_equal(a[k], b[k]) for k in a)


def rows_of(rows, ids):
    keep = np.isin(rows["user"], ids)
    return {k: rows[k][keep] for k in ("user", "item", "score", "cluster")}


def run_rows(ctx, conf, data, clustering=None, **kw):
    rec = pkg().RM2Job(conf, ctx).run(data, clustering=clustering, **kw)
    rows, st = rec.rows(), dict(rec.stats)
    rec.close()
    return rows, st


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- 1. the tiny shape against the dense statement
@pytest.mark.parametrize("top_n", [10, 1000])
@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("method,param", [("jm", 0.1), ("jm", 0.5), ("dirichlet", 50.0), ("absoluteDiscounting", 0.5), ("absoluteDiscounting", 1.0)])
def test_tiny_against_the_dense_statement(ctx, method, param, K, top_n):
    data, clustering, n_items = shape_data("tiny", K)
    if param == 1.0:
        assert int((data[2] <= 1.0).sum()) > 0          # ratings with r' = 0: still rated items
    ref = dense_reference("tiny", K, method, param)
    assert float(ref["rec_score"].min()) < -745.0       # rows whose unshifted likelihoods underflow exp()
    rows, st = run_rows(ctx, conf_of(method, param, n_items, K, top_n), data, clustering)
    worst = assert_topn_matches(rows, ref, top_n)
    print("%s %g, %d clusters, top %d: %d rows, worst relative error %.2e" % (method, param, K, top_n, len(rows["user"]), worst))
    assert st["recs"] == len(rows["user"]) > 0


# ---------------------------------------------------------------- 2. beta = 0: finite and infinite rows side by side
@pytest.mark.parametrize("method", ["jm", "dirichlet", "absoluteDiscounting"])
def test_hand_example_without_smoothing(ctx, method):
    rows, _ = run_rows(ctx, conf_of(method, 0.0, 5, 1, 10), HAND)
    got = {(int(a), int(b)): float(c) for a, b, c in zip(rows["user"], rows["item"], rows["score"])}
    want = {(1, 3): -5.493061, (1, 4): -5.075174, (4, 1): -3.583519}
    assert len(got) == 14
    for k, v in got.items():
        if k in want:
            assert abs(v - want[k]) <= RTOL * abs(want[k]), (k, v)
        else:
            assert v == -np.inf, (k, v)
    assert_topn_matches(rows, definition_full(*HAND, method, 0.0), 10)


def test_hand_example_with_smoothing(ctx):
    rows, _ = run_rows(ctx, conf_of("jm", 0.5, 5, 1, 10), HAND)
    got = {(int(a), int(b)): float(c) for a, b, c in zip(rows["user"], rows["item"], rows["score"])}
    assert len(got) == 14 and all(np.isfinite(v) for v in got.values())
    for k, v in {(1, 5): -4.526865, (4, 1): -2.783762}.items():
        assert abs(got[k] - v) <= RTOL * abs(v), (k, got[k])
    assert_topn_matches(rows, definition_full(*HAND, "jm", 0.5), 10)


@pytest.mark.parametrize("K", [1, 7])
def test_tiny_without_smoothing_is_all_minus_infinity(ctx, K):
    """no neighbour covers a user's items: every likelihood is 0"""
    data, clustering, n_items = shape_data("tiny", K)
    rows, _ = run_rows(ctx, conf_of("jm", 0.0, n_items, K, 10), data, clustering)
    ref = dense_reference("tiny", K, "jm", 0.0)
    assert len(rows["user"]) > 0 and np.all(np.isneginf(rows["score"])) and np.all(np.isneginf(ref["rec_score"]))
    assert_topn_matches(rows, ref, 10)


# ---------------------------------------------------------------- 3. the edge data of the RM2 tests
@pytest.mark.parametrize("method,param", [("jm", 0.5), ("dirichlet", 50.0), ("absoluteDiscounting", 0.5)])
def test_a_cluster_of_one_user(ctx, method, param):
    """user 9 alone in cluster 1, a user who rated every item of its cluster (no list), an unmapped user routed to cluster 0,
    scores <= 0 (dropped)"""
    user = np.array([1, 1, 2, 2, 3, 3, 4, 4, 4, 9, 9], dtype=np.int32)
    item = np.array([1, 2, 2, 3, 1, 3, 1, 2, 3, 5, 6], dtype=np.int32)
    score = np.array([5, 3, 4, 1, 2, 2, 0.5, 0, -1, 3, 0.5], dtype=np.float32)
    cl = (np.array([1, 2, 3, 4, 9], dtype=np.int32), np.array([2, 2, 2, 0, 1], dtype=np.int32))
    rows, _ = run_rows(ctx, conf_of(method, param, 6, 3, 10), (user, item, score), cl)
    ref = definition_full(user, item, score, method, param, clustering=cl)
    assert len(ref["rec_user"]) > 0
    assert_topn_matches(rows, ref, 10)
    assert 9 not in set(rows["user"].tolist()) and 4 not in set(rows["user"].tolist())
    assert np.all(np.isneginf(rows["score"][rows["cluster"] == 1]))


# ---------------------------------------------------------------- 4. a shape with more than one workgroup per product
def test_ml100k_in_one_cluster_against_the_dense_statement(ctx):
    data, clustering, n_items = shape_data("ml100k", 1)
    rows, st = run_rows(ctx, conf_of("jm", 0.1, n_items, 1, 50), data, clustering)
    ref = dense_reference("ml100k", 1, "jm", 0.1)
    worst = assert_topn_matches(rows, ref, 50)
    print("ML-100K shape, one cluster: %d rows of %d candidates, worst relative error %.2e; ms %s"
          % (len(rows["user"]), len(ref["rec_user"]), worst, {k: round(v, 2) for k, v in st.items() if k.startswith("ms_")}))
    assert len(rows["user"]) == 943 * 50


# ---------------------------------------------------------------- 5. chunks, batches, the workspace
@pytest.mark.parametrize("K", [1, 7])
def test_chunks_and_batches_do_not_change_a_bit(K, monkeypatch):
    P = pkg()
    data, clustering, n_items = shape_data("tiny", K)
    conf = conf_of("dirichlet", 50.0, n_items, K, 20)
    c0 = P.Context(0)
    base, st0 = run_rows(c0, conf, data, clustering)
    c0.close()
    monkeypatch.setenv("FY_RM1_NBR_CHUNK", "7")       # divides neither 200 users nor the cluster sizes of the 7-cluster split
    monkeypatch.setenv("FY_RM1_COL_CHUNK", "13")      # ... nor the item counts
    c1 = P.Context(0)
    per_user_most = 200 * 8 + 512 * 4
    forced, st1 = run_rows(c1, conf, data, clustering, workspace_bytes=2 * per_user_most)      # two or three users per batch (a tile holds eight)
    # cooc_launches = batches.  A score row is at least 256 floats, so a batch holds at most 2 * 3648 / 1024 = 7 of the 200 users
    assert st0["cooc_launches"] <= K and st1["cooc_launches"] >= -(-200 // 7)
    if K == 1:
        assert st1["cooc_launches"] == 100
    assert same_bits(forced, base)
    assert_topn_matches(forced, dense_reference("tiny", K, "dirichlet", 50.0), 20)
    # a workspace too small for one user's own rows
    with pytest.raises(RuntimeError, match="workspace_bytes") as info:
        P.RM2Job(conf, c1).run(data, clustering=clustering, workspace_bytes=1000)
    assert info.value.__cause__.code == -4 and "user" in str(info.value)
    again, _ = run_rows(c1, conf, data, clustering)
    assert same_bits(again, base)
    c1.close()


# ---------------------------------------------------------------- 6. requests
def check_requests(ctx, shape, K, top_n, method="jm", param=0.1):
    P = pkg()
    data, clustering, n_items = shape_data(shape, K)
    job = P.RM2Job(conf_of(method, param, n_items, K, top_n), ctx).prepare(data, clustering=clustering)
    try:
        known = np.unique(data[0][data[2] > 0]).astype(np.int32)
        first = job.score_users(known[3:4])               # a request before the full job
        full = job.score()
        frows = full.rows()
        assert same_bits(first.rows(), rows_of(frows, known[3:4])) and len(first.rows()["user"]) == top_n
        first.close()
        seventeen = known[np.linspace(0, len(known) - 1, 17).astype(int)]
        odd = np.array([known[3], known[3], 10 ** 9, -5, 0, known[-1], known[3]], dtype=np.int64).astype(np.int32)
        for ids in (seventeen, known[::-1], odd):
            a, b = job.score_users(ids), job.score_users(ids)
            want = rows_of(frows, ids)
            assert len(want["user"]) > 0 and same_bits(a.rows(), want) and same_bits(b.rows(), want)
            rq = a.request_stats
            assert rq["users_asked"] == len(ids) and rq["users_known"] == len(np.intersect1d(ids, known)) and rq["full_pass_clusters"] == 0
            assert a.stats["users_scored"] == len(np.unique(want["user"])) and a.stats["recs"] == len(want["user"])
            a.close()
            b.close()
        if K > 1:
            assert len(set(clustering[1][np.isin(clustering[0], seventeen)].tolist())) > 1      # the 17 users span clusters
        empty = job.score_users(np.array([10 ** 9], dtype=np.int32))
        assert len(empty.rows()["user"]) == 0
        empty.close()
        full.close()
        return frows
    finally:
        job.close()


@pytest.mark.parametrize("K", [1, 7])
def test_requests_are_the_rows_of_the_full_job_bit_for_bit(ctx, K):
    frows = check_requests(ctx, "tiny", K, 10)
    assert_topn_matches(frows, dense_reference("tiny", K, "jm", 0.1), 10)


def test_requests_on_the_ml1m_shape_in_50_clusters(ctx):
    frows = check_requests(ctx, "ml1m", 50, 50, "dirichlet", 100.0)
    assert len(np.unique(frows["user"])) == 6040 and np.all(np.isfinite(frows["score"]))


# ---------------------------------------------------------------- 7. filterUsers, a user with one rating
def test_filter_users_and_a_user_with_one_rating(ctx):
    (u, i, s), _, n_items = shape_data("tiny", 1)
    lone = int(u.max()) + 1
    u2, i2, s2 = np.append(u, lone).astype(np.int32), np.append(i, i[0]).astype(np.int32), np.append(s, 4.0).astype(np.float32)
    uu = np.unique(u2)
    cl = (uu, synth().hash_clustering(uu, 3))
    cut = int(np.median(uu))
    rows, st = run_rows(ctx, conf_of("jm", 0.1, n_items, 3, 10, filter_users=cut), (u2, i2, s2), cl)
    ref = definition_full(u2, i2, s2, "jm", 0.1, clustering=cl)
    keep = ref["rec_user"] >= cut                        # filtered users emit nothing and stay neighbours
    assert 0 < keep.sum() < len(keep)
    assert_topn_matches(rows, {k: v[keep] for k, v in ref.items()}, 10)
    assert rows["user"].min() >= cut and lone in set(rows["user"].tolist())
    assert st["users_scored"] == len(np.unique(rows["user"]))


# ---------------------------------------------------------------- 8. ranks
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("K", [1, 7])
def test_thread_ranks_equal_the_single_rank(ctx, world, K, monkeypatch):
    """1 cluster: replicated prep, the user loop sharded (the cooperative path is switched off: it is RM2's alone); 7 clusters:
    sharded prep, whole clusters per rank"""
    from test_rm2_smoothing_gpu import run_thread_ranks
    monkeypatch.setenv("FY_COOP", "0")
    data, clustering, n_items = shape_data("ml100k", K)
    conf = conf_of("absoluteDiscounting", 0.5, n_items, K, 20)
    single, _ = run_rows(ctx, conf, data, clustering)
    out, err = run_thread_ranks(world, data, clustering, conf, True)
    for e in err:
        if e is not None and not isinstance(e, threading.BrokenBarrierError):
            raise e
    assert all(len(o["user"]) > 0 for o in out)
    rows = {k: np.concatenate([o[k] for o in out]) for k in ("user", "item", "score", "cluster")}
    assert len(rows["user"]) == len(single["user"]) == 943 * 20
    order = np.lexsort((np.arange(len(rows["user"])), rows["user"]))
    sorder = np.lexsort((np.arange(len(single["user"])), single["user"]))
    assert same_bits({k: rows[k][order] for k in rows}, {k: single[k][sorder] for k in single})


def test_the_cooperative_path_refuses_rm1(ctx, monkeypatch):
    for k, v in (("FY_PRUNE_MIN_ITEMS", "256"), ("FY_M24_MIN_ITEMS", "0"), ("FY_SEED_CHUNKS", "1"), ("FY_COOP_FORCE", "1")):
        monkeypatch.setenv(k, v)
    P = pkg()
    par = __import__("importlib").import_module("filmyou-core_amd.parallel")
    data, clustering, n_items = shape_data("ml100k", 1)
    comm = par.ThreadCollectives(par.ThreadGroup(1), 0, 0)
    with pytest.raises(RuntimeError, match="cooperatively") as info:
        P.RM2Job(conf_of("jm", 0.1, n_items, 1, 20), ctx).run(data, clustering=clustering, rank=0, world=1, collectives=comm)
    assert info.value.__cause__.code == -10          # FY_ERR_UNSUPPORTED
    assert "FY_RM2_ESTIMATOR_RM1" in str(info.value)
    monkeypatch.delenv("FY_COOP_FORCE")
    rows, _ = run_rows(ctx, conf_of("jm", 0.1, n_items, 1, 50), data, clustering)      # the context is still good
    assert_topn_matches(rows, dense_reference("ml100k", 1, "jm", 0.1), 50)


# ---------------------------------------------------------------- 9. the work model
@pytest.mark.parametrize("K", [1, 7])
def test_work_counts_recounted(ctx, K):
    """per scored user u of cluster c, the first product tests the nnz_c - n_u entries of the neighbours' rows
    against the user's rated set, the second gathers the nnz_c entries of the cluster's columns"""
    (u, i, s), (cu, cc), n_items = shape_data("tiny", K)
    rows, st = run_rows(ctx, conf_of("jm", 0.1, n_items, K, 10), (u, i, s), (cu, cc))
    keep = s > 0
    cl_of = dict(zip(cu.tolist(), cc.tolist()))
    cl = np.array([cl_of.get(int(a), 0) for a in u[keep]])
    users, n_u = np.unique(u[keep], return_counts=True)
    ucl = np.array([cl_of.get(int(a), 0) for a in users])
    nnz_c = np.bincount(cl, minlength=K)
    I_c = np.array([len(np.unique(i[keep][cl == c])) for c in range(K)])
    scored = n_u < I_c[ucl]
    assert st["users_scored"] == int(scored.sum()) == len(np.unique(rows["user"]))
    assert st["recs"] == int(np.minimum(10, I_c[ucl] - n_u)[scored].sum()) == len(rows["user"])
    assert st["pair_contribs"] == int((nnz_c[ucl] - n_u)[scored].sum())
    assert st["log_terms"] == int(nnz_c[ucl][scored].sum())
    assert st["nnz"] == int(keep.sum()) and st["ms_total"] > 0 and st["ms_cooc"] > 0 and st["ms_score"] > 0 and st["ms_topn"] > 0
    assert st["cooc_launches"] == st["score_launches"] == int((nnz_c > 0).sum())


# ---------------------------------------------------------------- 10. the flag changes nothing else
def test_rm2_jobs_around_an_rm1_job_keep_their_bits(ctx):
    P = pkg()
    data, clustering, n_items = shape_data("ml100k", 7)
    kept = P.Ratings(ctx, *data)
    for method, param in (("jm", 0.1), ("dirichlet", 100.0)):
        rm2, rm1 = conf_of(method, param, n_items, 7, 20, model="rm2"), conf_of(method, param, n_items, 7, 20)
        before = P.RM2Job(rm2, ctx).run(kept, clustering=clustering)
        one = P.RM2Job(rm1, ctx).run(kept, clustering=clustering)
        after = P.RM2Job(rm2, ctx).run(kept, clustering=clustering)
        assert one.stats["prepared_from_cache"] == 1 and after.stats["prepared_from_cache"] == 1      # the kept state does not depend on the flag
        assert same_bits(before.rows(), after.rows())
        assert not np.array_equal(one.rows()["score"], before.rows()["score"])
        sa, sb = one.sums(), before.sums()
        assert sa.keys() == sb.keys() and all(np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])) for k in sa)
        fresh = P.RM2Job(rm1, ctx).run(data, clustering=clustering, cache=False)
        assert same_bits(fresh.rows(), one.rows())
        for r in (before, one, after, fresh):
            r.close()
    kept.close()


# ---------------------------------------------------------------- 11. the evaluator takes an RM1 result
def test_evaluator_takes_an_rm1_result(ctx):
    from test_eval_gpu import assert_equals_statement, fixture, split_fixture
    P = pkg()
    g = fixture()
    train, test, want_test = split_fixture(P, ctx, g)
    E = P.Evaluator(ctx, test, cutoffs=(1, 5, 10), relevance_threshold=4.0, coverage=True)
    conf = conf_of("jm", 0.5, g["numberOfItems"], g["numberOfClusters"], 1000)
    rec = P.RM2Job(conf, ctx).run(train, clustering=g["map"], clustering_count=g["clusteringCount"])
    rows = rec.rows()
    ev = E.evaluate(rec, per_user=True)
    want = eval_ref.evaluate(rows["user"], rows["item"], want_test, (1, 5, 10), 4.0, coverage=True)
    print("RM1 hits", ev.hits.tolist(), "of", ev.users_evaluated, "users")
    assert_equals_statement(ev, want, True)
    assert ev.users_evaluated == 30
    for x in (rec, E, train, test):
        x.close()


# ---------------------------------------------------------------- 13. the C entry points
def test_c_abi_flag_bits(ctx):
    P = pkg()
    native = P._native
    lib = native.load()
    data, _, n_items = shape_data("tiny", 1)
    ratings = P.Ratings(ctx, *data)
    out = C.c_void_p()
    for flags, lam, word in ((14, 1.0, b"both"), (10, -1.0, b"mu"), (12, float("inf"), b"delta"), (8, 1.5, b"lambda"), (16, 0.1, b"unknown"),
                             (8 | 32, 0.1, b"unknown")):
        p = native.RM2Params(lam, n_items, 10, 0, 1, 0, 1, flags, 0)
        assert lib.fy_rm2_prepare(ctx._h, C.byref(p), ratings._h, 0, None, None, None, C.byref(out)) == -1, (flags, lam)
        assert word in lib.fy_last_error(), lib.fy_last_error()
    for flags, lam in ((8, 0.0), (8, 1.0), (9, 0.5), (10, 100.0), (12, 0.5), (13, 7.5)):
        p = native.RM2Params(lam, n_items, 10, 0, 1, 0, 1, flags, 0)
        assert lib.fy_rm2_prepare(ctx._h, C.byref(p), ratings._h, 0, None, None, None, C.byref(out)) == 0, lib.fy_last_error()
        lib.fy_rm2_job_destroy(out)
    ratings.close()
    with pytest.raises(ValueError, match="relevanceModel"):
        P.RM2Job(conf_of("jm", 0.1, n_items, 1, 10, model="rm3"), ctx).run(data)
