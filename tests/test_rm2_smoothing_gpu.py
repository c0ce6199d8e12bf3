"""Dirichlet-prior and absolute-discounting smoothing of the RM2 job on the GPU, every flow a Jelinek-Mercer job can take.

Yardstick: tests/rm2_smoothing_definition.py -- the dense statement of the three methods (every candidate of every user, pinned to
the reference's estimator through oracle.rm2 in tests/test_rm2_smoothing_cpu.py) where the dense matrices fit, its rows-only
evaluator in torch fp64 for the emitted rows of the larger shapes.  Criterion: util.RTOL = 1e-5, purely relative, through
util.assert_topn_matches (dense) or fp64_definition.compare_with_definition (rows).  The tests that force the 24-bit matrix format
onto small data (FY_M24_MIN_ITEMS=0) pass atol=ATOL like the forced Jelinek-Mercer tests do -- small clusters keep fp32 rows in
production because their scores nearly cancel -- and print how many comparisons needed it."""
import ctypes as C
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

from fp64_definition import compare_with_definition
from rm2_smoothing_definition import definition_full, definition_rows
from test_rm2_smoothing_cpu import equal_rating_data, equal_sum_data
from util import ATOL, RTOL, assert_topn_matches, pkg, synth

pytestmark = pytest.mark.gpu

KEY = {"jm": "lambda", "dirichlet": "mu", "absoluteDiscounting": "delta"}


def conf_of(method, param, n_items, K, top_n):
    conf = pkg().Configuration()
    conf.set("smoothing", method)
    conf.set(KEY[method], repr(float(param)))
    conf.setInt("numberOfItems", n_items)
    conf.setInt("numberOfClusters", K)
    conf.setInt("numberOfRecommendations", top_n)
    return conf


@functools.lru_cache(maxsize=None)
def shape_data(shape, K):
    S = synth()
    u, i, s, facts = S.generate(shape)
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    uu = np.unique(u)
    return (u, i, s), (uu, S.hash_clustering(uu, K)), facts["n_items"]


@functools.lru_cache(maxsize=None)
def dense_reference(shape, K, method, param, n_items_conf=None):
    data, clustering, n_items = shape_data(shape, K)
    return definition_full(*data, method, param, n_items_conf or n_items, clustering=clustering)


def bits(rows):
    return {k: (rows[k].view(np.int32) if k == "score" else rows[k]) for k in ("user", "item", "score", "cluster")}


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return all(np.array_equal(a[k], b[k]) for k in a)


def needed_atol(rows, ref):
    want = {(int(a), int(b)): float(c) for a, b, c in zip(ref["rec_user"], ref["rec_item"], ref["rec_score"])}
    w = np.array([want[(int(a), int(b))] for a, b in zip(rows["user"], rows["item"])])
    g = rows["score"].astype(np.float64)
    fin = np.isfinite(w)
    return int(np.sum(np.abs(g[fin] - w[fin]) > RTOL * np.abs(w[fin])))


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- 1. edge cases
@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("method,param", [("dirichlet", 0.0), ("dirichlet", 50.0), ("absoluteDiscounting", 0.0), ("absoluteDiscounting", 0.5),
                                          ("absoluteDiscounting", 1.0)])
def test_edge_parameters_on_the_tiny_shape(ctx, K, method, param):
    """delta = 1.0 leaves ratings with r' = 0 (they stay rated items); mu = 0 and delta = 0 are Jelinek-Mercer with lambda = 0, -inf rows
    included"""
    P = pkg()
    data, clustering, n_items = shape_data("tiny", K)
    if method == "absoluteDiscounting" and param == 1.0:
        assert int((data[2] <= 1.0).sum()) > 0
    rec = P.RM2Job(conf_of(method, param, n_items, K, 10), ctx).run(data, clustering=clustering)
    rows = rec.rows()
    worst = assert_topn_matches(rows, dense_reference("tiny", K, method, param), 10)
    print("%s %g, %d clusters: %d rows, worst relative error %.2e" % (method, param, K, len(rows["user"]), worst))
    if param == 0.0:
        jm = P.RM2Job(conf_of("jm", 0.0, n_items, K, 10), ctx).run(data, clustering=clustering).rows()
        assert np.array_equal(rows["user"], jm["user"]) and np.array_equal(rows["item"], jm["item"])
        fin = np.isfinite(jm["score"])
        assert (~fin).sum() > 0 and np.array_equal(np.isfinite(rows["score"]), fin) and np.array_equal(rows["score"][~fin], jm["score"][~fin])
        assert np.all(np.abs(rows["score"][fin].astype(np.float64) - jm["score"][fin]) <= RTOL * np.abs(jm["score"][fin]))
    rec.close()


@pytest.mark.parametrize("method,param", [("jm", 0.5), ("dirichlet", 50.0), ("absoluteDiscounting", 0.5)])
def test_a_cluster_of_one_user(ctx, method, param):
    """The edge data of the Jelinek-Mercer tests: user 9 alone in cluster 1, a user who rated every item of its cluster (no list), an
    unmapped user routed to cluster 0, scores <= 0 (dropped).  A cluster's items are those its own users rated, so the lone user has
    no candidate and emits nothing, under every method; whatever a one-user cluster emitted would be -inf (every inner sum is 0)."""
    P = pkg()
    user = np.array([1, 1, 2, 2, 3, 3, 4, 4, 4, 9, 9], dtype=np.int32)
    item = np.array([1, 2, 2, 3, 1, 3, 1, 2, 3, 5, 6], dtype=np.int32)
    score = np.array([5, 3, 4, 1, 2, 2, 0.5, 0, -1, 3, 0.5], dtype=np.float32)
    cl = (np.array([1, 2, 3, 4, 9], dtype=np.int32), np.array([2, 2, 2, 0, 1], dtype=np.int32))
    rec = P.RM2Job(conf_of(method, param, 6, 3, 10), ctx).run((user, item, score), clustering=cl)
    rows = rec.rows()
    ref = definition_full(user, item, score, method, param, 6, clustering=cl)
    if len(ref["rec_user"]):
        assert_topn_matches(rows, ref, 10)
    else:
        assert len(rows["user"]) == 0
    # the one-user cluster: its user rated every item of the cluster, so it emits nothing -- and anything it did emit would be -inf
    alone = rows["cluster"] == 1
    assert np.all(np.isneginf(rows["score"][alone]))
    assert 9 not in set(ref["rec_user"].tolist()) or np.all(np.isneginf(ref["rec_score"][ref["rec_user"] == 9]))
    rec.close()


# ---------------------------------------------------------------- 2. the identities
def all_rows(ctx, data, cl, conf):
    rec = pkg().RM2Job(conf, ctx).run(data, clustering=cl)
    r = rec.rows()
    rec.close()
    return {(int(a), int(b)): float(c) for a, b, c in zip(r["user"], r["item"], r["score"])}


def assert_close_rows(a, b):
    assert a.keys() == b.keys() and len(a) > 0
    worst = 0.0
    for k, w in b.items():
        if np.isfinite(w):
            worst = max(worst, abs(a[k] - w) / abs(w))
        else:
            assert a[k] == w
    assert worst <= RTOL, worst
    return worst


@pytest.mark.parametrize("K", [1, 3])
def test_identity_equal_rating_sums_on_the_gpu(ctx, K):
    """every rating sum is 12: the Dirichlet rows are the Jelinek-Mercer rows of the same library at lambda = mu / (12 + mu)"""
    u, i, s, total = equal_sum_data(300, 400)
    cl = (np.arange(1, 301, dtype=np.int32), (np.arange(300) % K).astype(np.int32))
    for mu in (3.0, 50.0):
        a = all_rows(ctx, (u, i, s), cl, conf_of("dirichlet", mu, 400, K, 400))
        b = all_rows(ctx, (u, i, s), cl, conf_of("jm", mu / (total + mu), 400, K, 400))
        print("mu = %g, %d clusters: %d rows, worst relative difference %.2e" % (mu, K, len(a), assert_close_rows(a, b)))


@pytest.mark.parametrize("K", [1, 3])
def test_identity_equal_ratings_on_the_gpu(ctx, K):
    """every rating is 3: the absolute-discounting rows are the Jelinek-Mercer rows at lambda = delta / 3"""
    u, i, s, r0 = equal_rating_data(300, 400)
    cl = (np.arange(1, 301, dtype=np.int32), (np.arange(300) % K).astype(np.int32))
    for delta in (0.5, 2.0):
        a = all_rows(ctx, (u, i, s), cl, conf_of("absoluteDiscounting", delta, 400, K, 400))
        b = all_rows(ctx, (u, i, s), cl, conf_of("jm", delta / r0, 400, K, 400))
        print("delta = %g, %d clusters: %d rows, worst relative difference %.2e" % (delta, K, len(a), assert_close_rows(a, b)))


# ---------------------------------------------------------------- 3. the default small-cluster path
@pytest.mark.parametrize("method,param", [("dirichlet", 100.0), ("absoluteDiscounting", 0.5)])
def test_ml1m_in_50_clusters_against_the_rows_definition(ctx, method, param):
    data, clustering, n_items = shape_data("ml1m", 50)
    rec = pkg().RM2Job(conf_of(method, param, n_items, 50, 50), ctx).run(data, clustering=clustering)
    rows = rec.rows()
    ref = definition_rows(data, rows, method, param, n_items, clustering=clustering, device="cuda:0")
    out = compare_with_definition(rows, ref, rtol=RTOL)
    print("%s %g, ML-1M shape in 50 clusters: %d rows, worst relative error %.2e, %d over" % (method, param, out["rows"], out["worst"], out["n_over"]))
    assert out["rows"] > 250_000 and out["n_over"] == 0, out["worst_rows"]
    rec.close()


# ---------------------------------------------------------------- 4. the default packed path
@functools.lru_cache(maxsize=None)
def sampled_ml25m():
    S = synth()
    rng = np.random.Generator(np.random.PCG64(123))
    users = np.sort(rng.choice(S.SHAPES["ml25m"][0], size=400, replace=False)) + 1
    u, i, s, _ = S.generate("ml25m", users=users)
    return u.numpy(), i.numpy(), s.numpy()


PACKED_CASES = [("dirichlet", 100.0), ("dirichlet", 2000.0), ("absoluteDiscounting", 0.5)]


@functools.lru_cache(maxsize=None)
def packed_jobs(method, param):
    """(rows, stats, rows-definition comparison) of the sampled ML-25M cluster, N = 300: the default job, and the same job through
    the branch and bound (forced onto this 400-user neighbourhood; production prunes clusters of >= 600 users)"""
    P = pkg()
    u, i, s = sampled_ml25m()
    assert len(np.unique(i)) > 8192
    conf = conf_of(method, param, 59047, 1, 300)
    out = {}
    old = {k: os.environ.get(k) for k in ("FY_PRUNE_MIN_USERS", "FY_MAX_SURV_FRAC")}
    try:
        for name, env in (("plain", {}), ("pruned", {"FY_PRUNE_MIN_USERS": "0", "FY_MAX_SURV_FRAC": "1.5"})):
            os.environ.update(env)
            ctx = P.Context(0)
            rec = P.RM2Job(conf, ctx).run((u, i, s))
            rows, st = rec.rows(), dict(rec.stats)
            ref = definition_rows((u, i, s), rows, method, param, 59047, device="cuda:0")
            out[name] = (rows, st, compare_with_definition(rows, ref, rtol=RTOL))
            rec.close()
            ctx.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return out


@pytest.mark.parametrize("method,param", PACKED_CASES)
def test_packed_rows_and_the_branch_and_bound_on_sampled_ml25m_users(method, param):
    """400 users sampled from the ML-25M shape: about 22 000 items in one cluster, 24-bit rows without forcing.  Every emitted row of
    the default job and of the job through the branch and bound against the rows definition.  mu = 2000 shrinks the Gram part
    against the rank-one part by (s / (s + mu))^2."""
    jobs = packed_jobs(method, param)
    for name in ("plain", "pruned"):
        rows, st, out = jobs[name]
        print("%s %g, %s: %d rows, worst relative error %.2e, %d over; %d of %d blocks survive, %d fallbacks"
              % (method, param, name, out["rows"], out["worst"], out["n_over"], st["blocks_survived"], st["blocks_total"], st["prune_fallbacks"]))
        assert out["rows"] == 400 * 300 and out["n_over"] == 0, out["worst_rows"]
    assert jobs["plain"][1]["blocks_total"] == 0
    assert jobs["pruned"][1]["blocks_total"] > 0 and jobs["pruned"][1]["prune_fallbacks"] == 0


@pytest.mark.parametrize("method,param", PACKED_CASES)
def test_branch_and_bound_rows_are_the_unpruned_rows_bit_for_bit(method, param):
    """The rows of the job through the branch and bound against the rows of the default job, exactly.  Both flows score the matrix of
    the symmetric walk (a general-smoothing job never takes the full walk, whose elements below the diagonal are summed from the
    other row's fp32 weights: fy_rm2_plan.hpp), and the scoring kernels add whole batches of eight log terms exactly in fp64, so the
    grouping of the batches over waves does not show."""
    jobs = packed_jobs(method, param)
    a, b = jobs["pruned"][0], jobs["plain"][0]
    assert np.array_equal(a["user"], b["user"]) and len(a["score"]) == len(b["score"])
    moved = int(np.sum(a["item"] != b["item"]))
    differ = a["score"].view(np.int32) != b["score"].view(np.int32)
    rel = np.abs(a["score"].astype(np.float64) - b["score"]) / np.abs(b["score"].astype(np.float64))
    print("%s %g: %d of %d scores differ in their bits, largest relative difference %.2e, %d rows name another item"
          % (method, param, int(differ.sum()), len(differ), float(rel.max()), moved))
    assert same_bits(a, b)


# ---------------------------------------------------------------- 5. forced flows
FORCED = (("FY_PRUNE_MIN_ITEMS", "256"), ("FY_M24_MIN_ITEMS", "0"), ("FY_SEED_CHUNKS", "1"))
M_CANCEL = 40_000      # a numberOfItems that makes the scores of this shape cross zero: rows for the refinement pass


@pytest.mark.parametrize("refine", ["0", "1"])
@pytest.mark.parametrize("method,param", [("dirichlet", 100.0), ("absoluteDiscounting", 0.5)])
def test_forced_branch_and_bound_with_and_without_the_refinement_pass(method, param, refine, monkeypatch):
    for k, v in FORCED:
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("FY_REFINE", refine)
    P = pkg()
    data, clustering, _ = shape_data("ml100k", 3)
    ctx = P.Context(0)
    rec = P.RM2Job(conf_of(method, param, M_CANCEL, 3, 30), ctx).run(data, clustering=clustering)
    rows, st = rec.rows(), dict(rec.stats)
    ref = dense_reference("ml100k", 3, method, param, M_CANCEL)
    # (atol: the 24-bit format forced onto clusters of 1 400 items whose scores cross zero, as in test_refinement_of_rows_that_nearly_cancel)
    worst = assert_topn_matches(rows, ref, 30, atol=ATOL)
    print("%s %g, FY_REFINE=%s: worst relative error %.2e, %d of %d comparisons needed the absolute term, %d rows re-scored, %d of %d blocks"
          % (method, param, refine, worst, needed_atol(rows, ref), len(rows["user"]), st["rows_refined"], st["blocks_survived"], st["blocks_total"]))
    assert st["blocks_total"] > 0 and st["blocks_survived"] < st["blocks_total"]
    assert (st["rows_refined"] > 0) == (refine == "1")
    ctx.close()


@pytest.mark.parametrize("method,param", [("dirichlet", 100.0), ("absoluteDiscounting", 0.5)])
def test_forced_panel_mode(method, param, monkeypatch):
    for k, v in FORCED + (("FY_PANEL_MIN_CLUSTERS", "1"), ("FY_PANEL_COLS", "256"), ("FY_COOC_MAX_CH", "256")):
        monkeypatch.setenv(k, v)
    P = pkg()
    data, clustering, n_items = shape_data("ml100k", 3)
    ctx = P.Context(0)
    rec = P.RM2Job(conf_of(method, param, n_items, 3, 20), ctx).run(data, clustering=clustering)
    rows, st = rec.rows(), dict(rec.stats)
    ref = dense_reference("ml100k", 3, method, param)
    worst = assert_topn_matches(rows, ref, 20, atol=ATOL)      # (atol: the forced 24-bit format, as above)
    print("%s %g, panel mode: worst relative error %.2e, %d comparisons needed the absolute term, %d panel clusters, %d stray blocks"
          % (method, param, worst, needed_atol(rows, ref), st["panel_clusters"], st["stray_blocks"]))
    assert st["panel_clusters"] > 0
    ctx.close()


# ---------------------------------------------------------------- 6. requests
@pytest.mark.parametrize("side", ["2", "0"])       # FY_REQ_FULL_SHARE: the restricted pass / the full-pass fallback
@pytest.mark.parametrize("K", [1, 50])
@pytest.mark.parametrize("method,param", [("dirichlet", 100.0), ("absoluteDiscounting", 0.5)])
def test_requests_are_the_rows_of_the_full_job(ctx, method, param, K, side, monkeypatch):
    """the criterion of tests/test_rm2_request_gpu.py: the request's rows against the definition's rows of the requested users at RTOL,
    purely relative, with the row counts; on the full-pass side also bit for bit the full job's rows"""
    from test_rm2_request_gpu import check, expected
    monkeypatch.setenv("FY_REQ_FULL_SHARE", side)
    P = pkg()
    data, clustering, n_items = shape_data("ml100k", K)
    ref = dense_reference("ml100k", K, method, param)
    job = P.RM2Job(conf_of(method, param, n_items, K, 50), ctx).prepare(data, clustering=clustering)
    try:
        known = np.unique(data[0][data[2] > 0]).astype(np.int32)
        full = job.score()
        frows = full.rows()
        assert_topn_matches(frows, ref, 50)
        for ids in (known[5:6], known[10:80:10], known):
            rec = job.score_users(ids)
            check(rec, expected(ref, ids), 50)
            rq = rec.request_stats
            assert (rq["full_pass_clusters"] > 0) == (side == "0") and (rq["slab_rows"] > 0) == (side == "2")
            if side == "0":     # the full pass: bit for bit the full job's rows of these users, in its order
                keep = np.isin(frows["user"], ids)
                assert same_bits(rec.rows(), {k: frows[k][keep] for k in ("user", "item", "score", "cluster")})
            rec.close()
        full.close()
    finally:
        job.close()


# ---------------------------------------------------------------- 7. cache
def test_cache_key_holds_the_method_and_the_parameter(ctx):
    P = pkg()
    data, clustering, n_items = shape_data("ml100k", 7)
    jobs = [("jm", 0.1), ("dirichlet", 100.0), ("dirichlet", 200.0), ("dirichlet", 200.0), ("jm", 0.3), ("jm", 0.1), ("absoluteDiscounting", 0.5),
            ("jm", 0.1)]
    kept = P.Ratings(ctx, *data)
    previous = None
    for method, param in jobs:
        conf = conf_of(method, param, n_items, 7, 20)
        rec = P.RM2Job(conf, ctx).run(kept, clustering=clustering)
        fresh_ratings = P.Ratings(ctx, *data)
        fresh = P.RM2Job(conf, ctx).run(fresh_ratings, clustering=clustering)
        assert fresh.stats["prepared_from_cache"] == 0
        assert same_bits(rec.rows(), fresh.rows()), (method, param)
        sa, sb = rec.sums(), fresh.sums()
        assert all(np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])) for k in sa)
        # Jelinek-Mercer's kept state does not depend on lambda; the other methods' depends on (method, parameter)
        same_key = previous is not None and previous[0] == method and (method == "jm" or previous[1] == param)
        assert rec.stats["prepared_from_cache"] == (1 if same_key else 0), (previous, method, param)
        previous = (method, param)
        rec.close()
        fresh.close()
        fresh_ratings.close()
    kept.close()


def test_side_outputs_are_those_of_the_raw_ratings(ctx):
    P = pkg()
    data, clustering, n_items = shape_data("tiny", 7)
    base = P.RM2Job(conf_of("jm", 0.1, n_items, 7, 10), ctx).run(data, clustering=clustering).sums()
    for method, param in (("dirichlet", 100.0), ("absoluteDiscounting", 1.0)):
        got = P.RM2Job(conf_of(method, param, n_items, 7, 10), ctx).run(data, clustering=clustering).sums()
        assert got.keys() == base.keys()
        assert all(np.array_equal(np.asarray(got[k]), np.asarray(base[k])) for k in base)


# ---------------------------------------------------------------- 8. ranks
def run_thread_ranks(world, data, clustering, conf, use_collectives):
    """`world` threads of this process, one context each; the statistics through the library's collectives or through a host exchange"""
    P = pkg()
    par = __import__("importlib").import_module("filmyou-core_amd.parallel")
    group = par.ThreadGroup(world)
    out, err = [None] * world, [None] * world

    def body(rank):
        try:
            c = P.Context(0)
            rec = P.RM2Job(conf, c).run(data, clustering=clustering, rank=rank, world=world, collectives=par.ThreadCollectives(group, rank, 0))
            out[rank] = rec.rows()
            rec.close()
            c.close()
        except BaseException as e:
            err[rank] = e
            group.barrier.abort()

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not any(t.is_alive() for t in threads), "a rank is stuck"
    return out, err


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("K", [1, 7])
def test_thread_ranks_equal_the_single_rank(ctx, world, K, monkeypatch):
    """1 cluster: replicated prep, the user loop sharded (the cooperative path is switched off: it is Jelinek-Mercer's alone);
    7 clusters: sharded prep, whole clusters per rank"""
    monkeypatch.setenv("FY_COOP", "0")
    data, clustering, n_items = shape_data("ml100k", K)
    conf = conf_of("dirichlet", 100.0, n_items, K, 20)
    single = pkg().RM2Job(conf, ctx).run(data, clustering=clustering).rows()
    out, err = run_thread_ranks(world, data, clustering, conf, True)
    for e in err:
        if e is not None and not isinstance(e, threading.BrokenBarrierError):
            raise e
    rows = {k: np.concatenate([o[k] for o in out]) for k in ("user", "item", "score", "cluster")}
    assert len(rows["user"]) == len(single["user"])
    order = np.lexsort((np.arange(len(rows["user"])), rows["user"]))
    sorder = np.lexsort((np.arange(len(single["user"])), single["user"]))
    assert same_bits({k: rows[k][order] for k in rows}, {k: single[k][sorder] for k in single})


def test_the_cooperative_path_refuses_general_smoothing(ctx, monkeypatch):
    for k, v in FORCED + (("FY_COOP_FORCE", "1"),):
        monkeypatch.setenv(k, v)
    P = pkg()
    par = __import__("importlib").import_module("filmyou-core_amd.parallel")
    data, clustering, n_items = shape_data("ml100k", 1)
    comm = par.ThreadCollectives(par.ThreadGroup(1), 0, 0)
    with pytest.raises(RuntimeError, match="cooperatively") as info:
        P.RM2Job(conf_of("dirichlet", 100.0, n_items, 1, 20), ctx).run(data, clustering=clustering, rank=0, world=1, collectives=comm)
    assert info.value.__cause__.code == -10          # FY_ERR_UNSUPPORTED
    # the same job with Jelinek-Mercer takes the path, and the context is still good for a Dirichlet job without collectives
    rec = P.RM2Job(conf_of("jm", 0.1, n_items, 1, 20), ctx).run(data, clustering=clustering, rank=0, world=1, collectives=comm)
    assert rec.stats["blocks_total"] > 0
    rec.close()
    monkeypatch.delenv("FY_COOP_FORCE")
    rec = P.RM2Job(conf_of("dirichlet", 100.0, n_items, 1, 20), ctx).run(data, clustering=clustering)
    assert_topn_matches(rec.rows(), dense_reference("ml100k", 1, "dirichlet", 100.0), 20, atol=ATOL)     # (atol: forced 24-bit format)
    rec.close()


# ---------------------------------------------------------------- the C entry points
def test_c_abi_refuses_bad_smoothing_parameters(ctx):
    P = pkg()
    native = P._native
    lib = native.load()
    data, _, n_items = shape_data("tiny", 1)
    ratings = P.Ratings(ctx, *data)
    out = C.c_void_p()
    for flags, lam, word in ((6, 1.0, b"both"), (2, -1.0, b"mu"), (2, float("nan"), b"mu"), (2, float("inf"), b"mu"), (4, -0.5, b"delta"),
                             (4, float("inf"), b"delta"), (0, 1.5, b"lambda"), (1, -0.1, b"lambda")):
        p = native.RM2Params(lam, n_items, 10, 0, 1, 0, 1, flags, 0)
        assert lib.fy_rm2_prepare(ctx._h, C.byref(p), ratings._h, 0, None, None, None, C.byref(out)) == -1, (flags, lam)
        assert word in lib.fy_last_error(), lib.fy_last_error()
    for flags, lam in ((2, 0.0), (2, 1e6), (4, 0.0), (4, 7.5), (3, 100.0), (5, 0.5)):       # valid, NO_CACHE included
        p = native.RM2Params(lam, n_items, 10, 0, 1, 0, 1, flags, 0)
        assert lib.fy_rm2_prepare(ctx._h, C.byref(p), ratings._h, 0, None, None, None, C.byref(out)) == 0, lib.fy_last_error()
        lib.fy_rm2_job_destroy(out)
    ratings.close()


# ---------------------------------------------------------------- 9. the C++ host
def test_cpp_driver_gives_the_python_rows(ctx, tmp_path):
    P = pkg()
    exe = P._native.build_host_driver()
    data, clustering, n_items = shape_data("tiny", 7)
    np.savetxt(tmp_path / "ratings.txt", np.c_[data[0], data[1], data[2]], fmt=["%d", "%d", "%.1f"])
    np.savetxt(tmp_path / "clustering.txt", np.c_[clustering[0], clustering[1]], fmt="%d")
    out = subprocess.run([exe, str(tmp_path / "ratings.txt"), str(tmp_path / "clustering.txt"), "0.1", str(n_items), "7", "10", "smoothing=dirichlet",
                          "mu=100"], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert out.returncode == 0, out.stderr
    got = np.array([l.split() for l in out.stdout.strip().splitlines()])
    rows = P.RM2Job(conf_of("dirichlet", 100.0, n_items, 7, 10), ctx).run(data, clustering=clustering).rows()
    assert len(got) == len(rows["user"]) > 0
    assert np.array_equal(got[:, 0].astype(np.int32), rows["user"]) and np.array_equal(got[:, 1].astype(np.int32), rows["item"])
    assert np.array_equal(got[:, 2].astype(np.float64).astype(np.float32).view(np.int32), rows["score"].view(np.int32))      # %.9g reads back exactly
    assert np.array_equal(got[:, 3].astype(np.int32), rows["cluster"])
    # an unknown name and a missing parameter are refused by the mirror as by the Python host
    for extra in (["smoothing=laplace"], ["smoothing=absoluteDiscounting"]):
        bad = subprocess.run([exe, str(tmp_path / "ratings.txt"), str(tmp_path / "clustering.txt"), "0.1", str(n_items), "7", "10"] + extra,
                             capture_output=True, text=True, timeout=300, env=dict(os.environ))
        assert bad.returncode == 1 and "smoothing" in bad.stderr, bad.stderr
