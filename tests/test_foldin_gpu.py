"""Fold-in of given profiles on standing factors (fy_foldin_*) on the GPU: the reference's own vectors, bit for
bit against the factorisation's H update, the numpy statement of tests/foldin_ref.py at every k and profile length where the kernel
takes another path, masks, the refined level against ClusterRefinementJob, independence of a profile from its neighbours, and the
whole way from a driver run to RM2 lists for profiles nobody has seen.

Clusters are compared only where the statement's two largest allowed values differ by more than 1e-9 relative -- and every test asserts
that this holds for EVERY profile it compares, so none is left out."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import factor_edge_inputs as FE
import foldin_ref as FR
import refine_ref as RR
from util import pkg

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factorization_test_data.json")
MARGIN = 1e-9


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def conf_of(**kw):
    c = pkg().Configuration()
    for k, v in kw.items():
        c.setInt(k, v)
    return c


def coo(A):
    A = np.array(A)
    i, u = np.nonzero(A > 0)
    return (u + 1).astype(np.int32), (i + 1).astype(np.int32), A[i, u].astype(np.float32)


def worst_relative(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(got - want) / np.abs(want)
    e[(got == want) | (np.isnan(got) & np.isnan(want))] = 0.0
    return float(np.max(e))


def assert_matches_statement(a, ref, label=""):
    """status, parents and clusters equal; factor rows to rtol 1e-10 (the project's fp64 tolerance, test_random_vs_oracle)"""
    H = a.factors()
    print("%s: %d profiles, worst relative error of the factor rows %.3e, smallest margin %.3e" % (
        label, len(a.labels), worst_relative(H, ref["H"]), min(ref["margin"]) if len(ref["margin"]) else np.inf))
    np.testing.assert_allclose(H, ref["H"], rtol=1e-10, atol=1e-300)
    assert a.labels.tolist() == ref["labels"].tolist()
    assert a.status.tolist() == ref["status"].tolist()
    compared = ref["status"] == FR.OK
    assert all(m > MARGIN for m, c in zip(ref["margin"], compared) if c), "the inputs must keep every compared profile off a tie"
    assert all(m > MARGIN for m, c in zip(ref["margin1"], compared) if c)
    assert a.parents.tolist() == ref["parents"].tolist()
    assert a.clusters.tolist() == ref["clusters"].tolist()


def assert_counters(st, ref, n):
    c = ref["counters"]
    assert (st["profiles_asked"], st["profiles_mine"]) == (n, n)
    assert (st["entries_out_of_range"], st["entries_superseded"], st["entries_removed"], st["entries_nonpositive"], st["items_composed"]) == (
        c["out_of_range"], c["superseded"], c["removed"], c["nonpositive"], c["composed"])
    by = [int((ref["status"] == s).sum()) for s in (FR.OK, FR.EMPTY, FR.NO_CLUSTER, FR.EMPTY_IN_PARENT)]
    assert [st["profiles_assigned"], st["profiles_empty"], st["profiles_no_cluster"], st["profiles_empty_in_parent"]] == by
    assert st["collisions"] == c["collisions"]


# ---------------------------------------------------------------- pinned: the reference's own vectors
@pytest.mark.parametrize("name,ppc", [("nmf", False), ("ppc", True)])
def test_reference_vectors(ctx, golden, name, ppc):
    P = pkg()
    d = golden[name]
    f = P.FoldIn(ctx, np.array(d["W_init"]), ppc=ppc, normalizationFrequency=12)
    a = f.assign(FR.profiles_of_columns(d["A"]), iterations=1, h0=np.array(d["H_init"]))
    H = a.factors()
    print("%s: worst difference to H_one %.2e" % (name, np.max(np.abs(H - np.array(d["H_one"])))))
    np.testing.assert_allclose(H, np.array(d["H_one"]), rtol=0, atol=1e-9)
    ref = FR.assign(np.array(d["W_init"]), FR.profiles_of_columns(d["A"]), iterations=1, ppc=ppc, f=12, h0=np.array(d["H_init"]))
    assert_matches_statement(a, ref, name)
    f.close()


# ---------------------------------------------------------------- bit for bit against the factorisation
@functools.lru_cache(maxsize=None)
def random_matrix():
    rng = np.random.default_rng(300200)
    n_users, n_items = 300, 200
    A = (rng.random((n_items, n_users)) < 0.15) * rng.integers(1, 11, (n_items, n_users)) * 0.5      # half stars, no pair twice
    A[rng.integers(0, n_items, n_users), np.arange(n_users)] = 3
    A[np.arange(n_items), rng.integers(0, n_users, n_items)] = 4
    return A


@pytest.mark.parametrize("k", [7, 65])
@pytest.mark.parametrize("ppc,f", [(False, 0), (True, 0), (True, -1)])
def test_one_iteration_is_the_factorisations_h_bitwise(ctx, k, ppc, f):
    P = pkg()
    A = random_matrix()
    n_items, n_users = A.shape
    rng = np.random.default_rng(k)
    H0, W0 = rng.random((n_users, k)) + 0.01, rng.random((n_items, k)) + 0.01
    H, _ = P.NMFDriver(conf_of(numberOfUsers=n_users, numberOfItems=n_items, numberOfClusters=k, numberOfIterations=1, normalizationFrequency=f),
                       ctx, ppc=ppc).run(coo(A), H0, W0)
    fold = P.FoldIn(ctx, W0, ppc=ppc, normalizationFrequency=f)
    got = fold.assign(FR.profiles_of_columns(A), iterations=1, first_iteration=1, h0=H0).factors()
    print("k %d ppc %d f %d: %d of %d values differ" % (k, ppc, f, int((got != H).sum()), H.size))
    assert np.array_equal(got, H)
    fold.close()


@pytest.mark.parametrize("k", [7, 65])
def test_three_iterations_are_three_chained_h_updates_bitwise(ctx, k):
    P = pkg()
    A = random_matrix()
    n_items, n_users = A.shape
    rng = np.random.default_rng(100 + k)
    H0, W0 = rng.random((n_users, k)) + 0.01, rng.random((n_items, k)) + 0.01
    driver = P.NMFDriver(conf_of(numberOfUsers=n_users, numberOfItems=n_items, numberOfClusters=k, numberOfIterations=1, normalizationFrequency=-1),
                         ctx, ppc=True)
    H = H0
    for _ in range(3):
        H, _ = driver.run(coo(A), H, W0)      # W0 again: the fold-in holds W fixed
    fold = P.FoldIn(ctx, W0, ppc=True, normalizationFrequency=-1)
    got = fold.assign(FR.profiles_of_columns(A), iterations=3, h0=H0).factors()
    assert np.array_equal(got, H)
    fold.close()


def test_first_iteration_decides_the_normalisation(ctx):
    P = pkg()
    A = random_matrix()
    rng = np.random.default_rng(22)
    W0 = rng.random((A.shape[0], 9)) + 0.01
    profiles = FR.profiles_of_columns(A)[:40]
    fold = P.FoldIn(ctx, W0, ppc=True, normalizationFrequency=2)
    on = fold.assign(profiles, iterations=1, first_iteration=2)
    off = fold.assign(profiles, iterations=1, first_iteration=1)
    assert_matches_statement(on, FR.assign(W0, profiles, iterations=1, first_iteration=2, ppc=True, f=2), "normalised")
    assert_matches_statement(off, FR.assign(W0, profiles, iterations=1, first_iteration=1, ppc=True, f=2), "not normalised")
    np.testing.assert_allclose(np.abs(on.factors()).sum(1), 1.0, rtol=1e-12)
    assert not np.allclose(np.abs(off.factors()).sum(1), 1.0)
    fold.close()


# ---------------------------------------------------------------- against the statement
LENGTHS = (1, 3, 4, 5, 511, 512, 513, 1025)      # the four-way tail, one chunk less / more one entry, three chunks


@functools.lru_cache(maxsize=None)
def length_profiles():
    rng = np.random.default_rng(1025)
    n_items = 1100
    out = []
    for label, n in enumerate(LENGTHS):
        items = rng.permutation(n_items)[:n] + 1                           # unsorted: the ingest orders them
        out.append((1000 + label, items, rng.integers(1, 11, n).astype(np.float32) * 0.5))
    return n_items, out


@pytest.mark.parametrize("k,ppc", [(1, True), (63, True), (64, True), (65, True), (128, True), (256, True), (65, False), (64, False)])
def test_every_k_and_length_vs_statement(ctx, k, ppc):
    """uniform start, 10 iterations; k on both sides of the LDS copy of C (64) and of every 64 columns of the register arrays"""
    P = pkg()
    n_items, profiles = length_profiles()
    rng = np.random.default_rng(7000 + k)
    W = rng.random((n_items, k)) + 0.01
    fold = P.FoldIn(ctx, W, ppc=ppc, normalizationFrequency=-1)
    a = fold.assign(profiles, iterations=10)
    ref = FR.assign(W, profiles, iterations=10, ppc=ppc, f=-1)
    assert_matches_statement(a, ref, "k %d ppc %d" % (k, ppc))
    assert_counters(a.foldin_stats, ref, len(profiles))
    assert a.foldin_stats["entries"] == sum(LENGTHS) == a.foldin_stats["items_composed"]
    fold.close()


def test_grid_stride_loop_wraps(ctx):
    """17 000 profiles of 1 to 3 items: more waves than one launch has (4096 blocks of four)"""
    P = pkg()
    rng = np.random.default_rng(17000)
    n, n_items, k = 17000, 50, 5
    W = rng.random((n_items, k)) + 0.01
    lens = rng.integers(1, 4, n)
    start = np.r_[0, np.cumsum(lens)].astype(np.int64)
    item = np.concatenate([rng.permutation(n_items)[:m] + 1 for m in lens]).astype(np.int32)
    score = (rng.integers(1, 11, len(item)) * 0.5).astype(np.float32)
    labels = np.arange(1, n + 1, dtype=np.int32)
    fold = P.FoldIn(ctx, W, ppc=True, normalizationFrequency=-1)
    a = fold.assign((labels, start, item, score), iterations=10)
    profiles = [(labels[p], item[start[p]:start[p + 1]], score[start[p]:start[p + 1]]) for p in range(n)]
    ref = FR.assign(W, profiles, iterations=10, ppc=True, f=-1)
    assert_matches_statement(a, ref, "wrap")
    assert_counters(a.foldin_stats, ref, n)
    fold.close()


def test_zero_iterations_return_the_start(ctx):
    P = pkg()
    n_items, profiles = length_profiles()
    rng = np.random.default_rng(5)
    k = 70
    W = rng.random((n_items, k))
    h0 = rng.random((len(profiles), k))
    counts = np.zeros(k, np.int32)
    counts[[3, 66]] = 1
    fold = P.FoldIn(ctx, W, ppc=True, counts=counts)
    a = fold.assign(profiles, iterations=0, h0=h0)
    assert np.array_equal(a.factors(), h0)
    assert a.clusters.tolist() == [3 if h0[p, 3] >= h0[p, 66] else 66 for p in range(len(profiles))]
    u = fold.assign(profiles, iterations=0)
    assert np.array_equal(u.factors(), np.full((len(profiles), k), 1.0 / k)) and (u.clusters == 3).all()      # the first ALLOWED index
    fold.close()


@pytest.mark.parametrize("iterations", [1, 2])
def test_infinities_are_clamped_like_the_factorisation(ctx, iterations):
    """One of factor_edge_inputs' overflowing matrices as W: W^T W is infinite everywhere, PPC's sums are clamped to DBL_MAX."""
    P = pkg()
    rng = np.random.default_rng(200)
    n_items, k = 40, 4
    W = FE.huge_initial(rng, (n_items, k))
    with np.errstate(over="ignore"):
        assert np.isinf(W.T @ W).all()
    profiles = [(p, rng.permutation(n_items)[:6] + 1, rng.integers(1, 6, 6).astype(np.float32)) for p in range(12)]
    h0 = rng.random((12, k)) + 0.5
    fold = P.FoldIn(ctx, W, ppc=True, normalizationFrequency=0)
    a = fold.assign(profiles, iterations=iterations, h0=h0)
    ref = FR.assign(W, profiles, iterations=iterations, ppc=True, f=0, h0=h0)
    assert np.isfinite(a.factors()).all() and np.isfinite(ref["H"]).all()
    assert_matches_statement(a, ref, "clamped")
    fold.close()


def test_a_nan_row_of_w_gives_no_cluster(ctx):
    P = pkg()
    rng = np.random.default_rng(8)
    W = rng.random((20, 6)) + 0.01
    W[4] = np.nan                                            # item 5
    profiles = [(1, [2, 5, 9], [1.0, 2.0, 3.0]), (2, [2, 9], [1.0, 3.0]), (3, [5], [4.0])]
    fold = P.FoldIn(ctx, W, ppc=False)
    a = fold.assign(profiles, iterations=3)
    # C = W^T W is NaN throughout, so every row is NaN: nobody has a cluster, and the statement says the same
    ref = FR.assign(W, profiles, iterations=3, ppc=False, f=-1)
    assert a.status.tolist() == ref["status"].tolist() == [FR.NO_CLUSTER] * 3
    assert (a.clusters == -1).all() and (a.parents == -1).all() and np.isnan(a.factors()).all()
    # zero iterations never read C: only the argmax of the start counts
    assert fold.assign(profiles, iterations=0).status.tolist() == [FR.OK] * 3
    fold.close()


# ---------------------------------------------------------------- masks
def test_masks_move_the_argmax_and_nothing_else(ctx):
    P = pkg()
    A = random_matrix()
    rng = np.random.default_rng(31)
    k = 12
    W = rng.random((A.shape[0], k)) + 0.01
    profiles = FR.profiles_of_columns(A)[:60]
    free = P.FoldIn(ctx, W, ppc=True)
    a = free.assign(profiles, iterations=10)
    ref = FR.assign(W, profiles, iterations=10, ppc=True, f=-1)
    assert_matches_statement(a, ref, "unmasked")
    counts = np.ones(k, np.int32)
    counts[np.unique(a.clusters)[:2]] = 0                    # two clusters that do win lose their residents
    moved = np.isin(a.clusters, np.flatnonzero(counts == 0))
    assert moved.any() and not moved.all()
    masked = P.FoldIn(ctx, W, ppc=True, counts=counts)
    b = masked.assign(profiles, iterations=10)
    refm = FR.assign(W, profiles, iterations=10, ppc=True, f=-1, counts=counts)
    assert_matches_statement(b, refm, "masked")
    assert np.array_equal(a.factors(), b.factors())                              # the mask never touches the iterations
    assert (counts[b.clusters] > 0).all() and np.array_equal(b.clusters[~moved], a.clusters[~moved]) and (b.clusters[moved] != a.clusters[moved]).all()
    nobody = P.FoldIn(ctx, W, ppc=True, counts=np.zeros(k, np.int32))
    c = nobody.assign(profiles, iterations=10)
    assert (c.status == FR.NO_CLUSTER).all() and (c.clusters == -1).all() and c.foldin_stats["profiles_no_cluster"] == len(profiles)
    for f in (free, masked, nobody):
        f.close()


# ---------------------------------------------------------------- the refined level
@functools.lru_cache(maxsize=None)
def three_parents():
    """60 users in parents of 4 (k_c = 1), 20 (k_c = 4) and 36 (k_c = 8) users, usersPerSubCluster = 5"""
    rng = np.random.default_rng(33)
    sizes = [4, 20, 36]
    n_users, n_items = sum(sizes), 45
    A = (rng.random((n_users, n_items)) < 0.25) * rng.integers(1, 11, (n_users, n_items)) * 0.5
    A[np.arange(n_users), rng.integers(0, n_items, n_users)] = 3
    u, i = np.nonzero(A)
    users = (rng.permutation(n_users) + 1).astype(np.int32)
    cl = np.repeat(np.arange(3), sizes).astype(np.int32)
    return (u + 1).astype(np.int32), (i + 1).astype(np.int32), A[u, i].astype(np.float32), users, cl, n_items


@pytest.mark.parametrize("f", [-1, 0])
def test_second_level_equals_the_refinement(ctx, f):
    P = pkg()
    u, i, s, mu, mc, n_items = three_parents()
    K, ups = 3, 5
    m = RR.mappings(u, i, s, mu, mc, K)
    kc = RR.sub_clusters(m, ups)
    assert kc == [1, 4, 8]
    rng = np.random.default_rng(44)
    H0 = [np.full((len(m["users"][c]), kc[c]), 1.0 / kc[c]) for c in range(K)]
    W0 = [rng.random((len(m["items"][c]), kc[c])) + 0.01 for c in range(K)]
    conf = conf_of(numberOfUsers=len(mu), numberOfClusters=K, usersPerSubCluster=ups, numberOfIterations=1, normalizationFrequency=f)
    job = P.ClusterRefinementJob(conf, ctx, ppc=True)
    users, clusters, counts = job.run((u, i, s), (mu, mc), H0=H0, W0=W0, keep_factors=True)
    maps = P.SubClusterMappingJob(conf, ctx).run((u, i, s), (mu, mc))
    stride = -(-len(mu) // K)
    Wtop = rng.random((n_items, K)) + 0.01
    for c in range(K):
        residents = np.asarray(m["users"][c])
        profiles = [(int(r), i[(u == r) & (s > 0)], s[(u == r) & (s > 0)]) for r in residents]
        onehot = np.zeros(K * stride, np.int32)
        onehot[c * stride:c * stride + kc[c]] = 1                       # pass 1 can only answer parent c
        fold = P.FoldIn(ctx, Wtop, ppc=True, normalizationFrequency=f).add_level(maps, W0, stride, counts=onehot)
        a = fold.assign(profiles, iterations=1)
        assert (a.parents == c).all() and (a.status == FR.OK).all()
        Hc = job.factors[c][0]
        sub = a.sub_factors()
        got = np.array(sub).reshape(len(residents), kc[c])
        print("parent %d k_c %d f %d: worst relative error to the refined H_c %.3e" % (c, kc[c], f, worst_relative(got, Hc)))
        np.testing.assert_allclose(got, Hc, rtol=1e-10, atol=1e-300)
        level = dict(items=[np.asarray(x) for x in m["items"]], W=W0, stride=stride, counts=onehot)
        ref = FR.assign(Wtop, profiles, iterations=1, ppc=True, f=f, level=level)
        assert_matches_statement(a, ref, "parent %d" % c)
        # the same ids the refinement gave its residents
        want = {int(x): int(y) for x, y in zip(users, clusters)}
        assert a.clusters.tolist() == [want[int(r)] for r in residents]
        assert a.foldin_stats["items_in_parent"] == ref["counters"]["in_parent"] == sum(len(p[1]) for p in profiles)
        fold.close()


def test_second_level_statuses_and_collisions(ctx):
    P = pkg()
    u, i, s, mu, mc, n_items = three_parents()
    K = 3
    m = RR.mappings(u, i, s, mu, mc, K)
    kc = [1, 4, 8]
    rng = np.random.default_rng(45)
    W0 = [rng.random((len(m["items"][c]), kc[c])) + 0.01 for c in range(K)]
    Wtop = rng.random((n_items + 5, K)) + 0.01                          # five items nobody of any parent rated
    maps = P.SubClusterMappingJob(conf_of(numberOfClusters=K), ctx).run((u, i, s), (mu, mc))
    outside = [n_items + 1, n_items + 3]
    inside = rng.permutation(np.asarray(m["items"][2]))[:7]
    profiles = [(1, outside, [4.0, 5.0]), (2, inside, rng.integers(1, 6, 7).astype(np.float32)),
                (3, np.r_[inside[:3], outside], [1.0, 2.0, 3.0, 4.0, 5.0]), (4, [0], [1.0])]
    level = dict(items=[np.asarray(x) for x in m["items"]], W=W0, stride=20, counts=None)
    fold = P.FoldIn(ctx, Wtop, ppc=True).add_level(maps, W0, 20)
    a = fold.assign(profiles, iterations=10)
    ref = FR.assign(Wtop, profiles, iterations=10, ppc=True, f=-1, level=level)
    assert_matches_statement(a, ref, "two levels")
    assert_counters(a.foldin_stats, ref, 4)
    assert a.status[0] == FR.EMPTY_IN_PARENT and a.parents[0] >= 0 and a.clusters[0] == -1 and len(a.sub_factors()[0]) == kc[a.parents[0]]
    assert a.status[3] == FR.EMPTY and len(a.sub_factors()[3]) == 0
    for p in range(4):
        np.testing.assert_allclose(a.sub_factors()[p], ref["H1"][p], rtol=1e-10, atol=1e-300)
    fold.close()
    # a stride smaller than some k_c: ids of neighbouring parents collide; counted, nothing renumbered
    big = [(10 + j, rng.permutation(np.asarray(m["items"][2]))[:9], rng.integers(1, 6, 9).astype(np.float32)) for j in range(30)]
    fold = P.FoldIn(ctx, Wtop, ppc=True).add_level(maps, W0, 2)
    b = fold.assign(big, iterations=10)
    level = dict(items=[np.asarray(x) for x in m["items"]], W=W0, stride=2, counts=None)
    refb = FR.assign(Wtop, big, iterations=10, ppc=True, f=-1, level=level)
    assert_matches_statement(b, refb, "collisions")
    assert b.foldin_stats["collisions"] == refb["counters"]["collisions"] > 0
    ok = b.status == FR.OK
    assert ok.any() and b.clusters[ok].tolist() == [int(b.parents[p]) * 2 + int(np.argmax(b.sub_factors()[p])) for p in np.flatnonzero(ok)]
    fold.close()


# ---------------------------------------------------------------- independence
def test_a_profiles_outputs_do_not_depend_on_its_neighbours(ctx):
    P = pkg()
    A = random_matrix()
    rng = np.random.default_rng(61)
    k = 65
    W = rng.random((A.shape[0], k)) + 0.01
    profiles = FR.profiles_of_columns(A)[:100]
    fold = P.FoldIn(ctx, W, ppc=True)
    whole = fold.assign(profiles, iterations=10)
    H = whole.factors()
    alone = fold.assign([profiles[37]], iterations=10)
    assert np.array_equal(alone.factors()[0], H[37]) and alone.clusters[0] == whole.clusters[37]
    order = rng.permutation(100)
    mixed = fold.assign([profiles[j] for j in order], iterations=10)
    assert np.array_equal(mixed.factors(), H[order]) and np.array_equal(mixed.clusters, whole.clusters[order])
    parts = [fold.assign(profiles, iterations=10, rank=r, world=3) for r in range(3)]
    assert [len(p.labels) for p in parts] == [33, 33, 34]
    assert np.array_equal(np.concatenate([p.factors() for p in parts]), H)
    for key in ("labels", "clusters", "parents", "status"):
        assert np.array_equal(np.concatenate([getattr(p, key) for p in parts]), getattr(whole, key)), key
    assert all(p.foldin_stats["profiles_asked"] == 100 for p in parts) and sum(p.foldin_stats["profiles_mine"] for p in parts) == 100
    fold.close()


# ---------------------------------------------------------------- refusals on a live model
def test_refusals_leave_the_model_usable(ctx):
    P = pkg()
    lib = P._native.load()
    rng = np.random.default_rng(2)
    W = rng.random((10, 3)) + 0.01
    fold = P.FoldIn(ctx, W, ppc=True)
    good = [(1, [1, 2], [1.0, 2.0])]
    want = fold.assign(good, iterations=2).factors()
    lab, item, score = np.array([1, 2], np.int32), np.array([1, 2, 3], np.int32), np.ones(3, np.float32)

    def code(fn):
        with pytest.raises(P.FilmYouError) as e:
            fn()
        return e.value.code

    assert code(lambda: fold.assign((lab, np.array([0, 2, 1], np.int64), item, score))) == -1       # start decreases
    assert code(lambda: fold.assign((lab, np.array([1, 2, 3], np.int64), item, score))) == -1       # start[0] != 0
    assert code(lambda: fold.assign(good, rank=1, world=1)) == -1 and code(lambda: fold.assign(good, rank=0, world=0)) == -1
    assert code(lambda: fold.assign(good, iterations=-1)) == -1 and code(lambda: fold.assign(good, first_iteration=-1)) == -1
    q, keep = P.host._itemcf_profiles(good, "resident", 0.0)
    out = C.c_void_p(1)
    assert lib.fy_foldin_assign(fold._h, C.byref(q), 1, 1, None, 0, 1, C.byref(out)) == -1 and out.value is None      # whole profiles only
    one = np.ones(3, np.int32)
    lists = np.array([1, 3, 2], np.int32)

    def level(n_parents, m_c, k_c, items, stride):
        m_c, k_c = np.asarray(m_c, np.int32), np.asarray(k_c, np.int32)
        w = np.ones(int((m_c * k_c).sum()) or 1)
        return lib.fy_foldin_add_level(fold._h, n_parents, m_c.ctypes.data, k_c.ctypes.data, items.ctypes.data, w.ctypes.data, stride, None, 0)
    assert level(2, [1, 1], [1, 1], lists, 1) == -1                                   # one block per top-level cluster
    assert level(3, [3, 0, 0], [1, 1, 1], lists, 1) == -1 and b"ascending" in lib.fy_last_error()
    assert level(3, [1, 1, 1], [1, 257, 1], one, 1) == -10                            # FY_ERR_UNSUPPORTED
    assert level(3, [1, 1, 1], [1, 1, 1], one, 0) == -1                               # stride
    assert np.array_equal(fold.assign(good, iterations=2).factors(), want)            # still the model it was
    assert level(3, [1, 1, 1], [1, 1, 1], one, 1) == 0 and level(3, [1, 1, 1], [1, 1, 1], one, 1) == -9      # a second level: FY_ERR_STATE
    empty = fold.assign([], iterations=2)
    assert len(empty.labels) == 0 and empty.factors().shape == (0, 3) and empty.sub_factors() == []
    fold.close()


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("users_per_sub_cluster", [-1, 12])
def test_driver_model_assigns_visitors_and_rm2_scores_them(ctx, users_per_sub_cluster):
    P = pkg()
    rng = np.random.default_rng(77)
    n_users, n_items, K = 120, 60, 4
    A = (rng.random((n_users + 15, n_items)) < 0.25) * rng.integers(1, 11, (n_users + 15, n_items)) * 0.5
    A[np.arange(len(A)), rng.integers(0, n_items, len(A))] = 3
    A[rng.integers(0, n_users, n_items), np.arange(n_items)] = 4
    u, i = np.nonzero(A[:n_users])
    conf = conf_of(numberOfUsers=n_users, numberOfItems=n_items, numberOfClusters=K, usersPerSubCluster=users_per_sub_cluster,
                   numberOfIterations=5, numberOfRecommendations=0)
    R = P.Ratings(ctx, (u + 1).astype(np.int32), (i + 1).astype(np.int32), A[u, i].astype(np.float32))
    try:
        driver = P.RMRecommenderDriver(conf, ctx)
        assert driver.fold_in is None
        _, (users, clusters, counts) = driver.run(R, seed=3, keep_model=True)
        plain = P.RMRecommenderDriver(conf, ctx)
        _, (users0, clusters0, counts0) = plain.run(R, seed=3)
        assert plain.fold_in is None and np.array_equal(clusters0, clusters) and np.array_equal(counts0, counts)      # the default changes nothing
        holdout = [(1000 + j, np.flatnonzero(A[n_users + j]) + 1, A[n_users + j][A[n_users + j] > 0].astype(np.float32)) for j in range(15)]
        holdout.append((2000, [], []))
        a = driver.fold_in.assign(holdout, iterations=5)
        ok = a.status == FR.OK
        assert a.status[-1] == FR.EMPTY and ok.sum() >= 10 and (counts[a.clusters[ok]] > 0).all()
        rm2_conf = conf_of(numberOfItems=n_items, numberOfClusters=len(counts), numberOfRecommendations=5)
        rm2_conf.setFloat("lambda", 0.5)
        prepared = P.RM2Job(rm2_conf, ctx).prepare(R, clustering=(users, clusters), clustering_count=counts)
        rec = prepared.score_profiles([holdout[j] for j in np.flatnonzero(ok)], base="whole", clusters=a.clusters[ok])
        rows = rec.rows()
        want = {int(l): int(c) for l, c in zip(a.labels[ok], a.clusters[ok])}
        assert set(rows["user"].tolist()) == set(want)
        assert all(want[int(l)] == int(c) for l, c in zip(rows["user"], rows["cluster"]))
        rec.close()
        prepared.close()
        driver.fold_in.close()
    finally:
        R.close()
