"""Cluster refinement on the GPU (fy_submap_*, fy_cluster_refine, RMRecommenderDriver): the mappings against a numpy restatement,
every parent's factors against oracle.nmf on its extracted submatrix, the refined clustering against the composition of the
oracles, the reference's failures, determinism, and the one-call driver against RM2Job and oracle.rm2 -- its PPC stage against
oracle.nmf and oracle.cluster_assign.  The inputs of factor_edge_inputs.py take the per-parent comparison to rows of several
chunks on both sides, in both branches of the SpMM, to wave loops that wrap and to the infinity clamps."""
import numpy as np
import pytest

import factor_edge_inputs as FE
import oracle
import refine_ref as RR
from util import assert_topn_matches, pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


def conf_of(**kw):
    c = pkg().Configuration()
    for k, v in kw.items():
        c.setInt(k, v)
    return c


# ---------------------------------------------------------------- mappings
def ragged_mapping_input(seed):
    rng = np.random.default_rng(seed)
    n_users, n_items, K = 90, 60, 5
    A = (rng.random((n_users, n_items)) < 0.2) * rng.integers(1, 6, (n_users, n_items))
    u, i = np.nonzero(A)
    s = A[u, i].astype(np.float32)
    u, i = u + 1, i + 1
    s[::7] = 0.0                                         # scores <= 0 are dropped ...
    s[3::11] = -2.0
    extra_u, extra_i = np.array([2, 2, 40]), np.array([n_items + 5, n_items + 9, n_items + 9])      # ... also when they are an item's only ratings
    u, i, s = np.r_[u, extra_u], np.r_[i, extra_i], np.r_[s, np.float32([0.0, -1.0, 0.0])]
    order = rng.permutation(len(u))                      # shuffled COO
    u, i, s = u[order].astype(np.int32), i[order].astype(np.int32), s[order].astype(np.float32)
    users = np.arange(1, n_users + 1)
    absent = np.array([5, 17, 33])                       # not in the map: their items land in cluster 0, they join no user map
    named = np.setdiff1d(users, absent)
    cl = rng.integers(0, K, len(named))
    cl[cl == 3] = 1                                      # cluster 3 stays empty
    cl[rng.random(len(named)) < 0.6] = 1                 # cluster 1 holds most users
    beyond = np.array([n_users + 30, n_users + 500])     # mapped users beyond every rated id (no rating at all)
    mu = np.r_[named, beyond, named[:6], [n_users + 30]]      # repeated entries: the later one wins
    mc = np.r_[cl, [2, 4], (cl[:6] + 1) % 3, [0]]
    return (u, i, s), mu.astype(np.int32), mc.astype(np.int32), K


@pytest.mark.parametrize("seed", [1, 2])
def test_mappings_match_the_numpy_restatement(ctx, seed):
    P = pkg()
    (u, i, s), mu, mc, K = ragged_mapping_input(seed)
    got = P.SubClusterMappingJob(conf_of(numberOfClusters=K), ctx).run((u, i, s), (mu, mc))
    m = RR.mappings(u, i, s, mu, mc, K)
    assert got.users_in_cluster.tolist() == [len(x) for x in m["users"]]
    assert got.items_in_cluster.tolist() == [len(x) for x in m["items"]]
    assert got.users_in_cluster[3] == 0 and got.users_in_cluster[1] == got.users_in_cluster.max()
    assert got.user.tolist() == np.concatenate(m["users"]).tolist()
    assert got.user_cluster.tolist() == np.repeat(np.arange(K), got.users_in_cluster).tolist()
    assert got.user_new_id.tolist() == np.concatenate([np.arange(1, len(x) + 1) for x in m["users"]]).tolist()
    assert got.item.tolist() == np.concatenate(m["items"]).tolist()
    assert got.item_cluster.tolist() == np.repeat(np.arange(K), got.items_in_cluster).tolist()
    assert got.item_new_id.tolist() == np.concatenate([np.arange(1, len(x) + 1) for x in m["items"]]).tolist()
    # the cases the input was built for
    assert not set([5, 17, 33]) & set(got.user.tolist())
    absent_items = set(i[np.isin(u, [5, 17, 33]) & (s > 0)].tolist())
    assert absent_items and absent_items <= set(m["items"][0].tolist())
    assert 120 in got.user.tolist() and 590 in got.user.tolist() and got.user_cluster[got.user.tolist().index(120)] == 0
    assert not set([65, 69]) & set(got.item.tolist())
    # the remapped kept ratings, both ways
    assert got.nnz == int(m["kept"].sum())
    vals = s[m["kept"]]
    for have, want in ((got.csr, RR.csr(m["row_user"], m["row_item"], vals, len(got.user))),
                       (got.csc, RR.csr(m["row_item"], m["row_user"], vals, len(got.item)))):
        for a, b in zip(have, want):
            assert np.array_equal(a, b)


def test_mappings_reject_what_the_stage_cannot_route(ctx):
    P = pkg()
    u = np.array([1, 2], np.int32)
    with pytest.raises(RuntimeError, match="outside"):
        P.SubClusterMappingJob(conf_of(numberOfClusters=2), ctx).run((u, u, np.ones(2, np.float32)), (u, np.array([0, 2], np.int32)))
    with pytest.raises(RuntimeError, match="negative"):
        P.SubClusterMappingJob(conf_of(numberOfClusters=2), ctx).run((u, u, np.ones(2, np.float32)), (np.array([1, -4], np.int32), np.array([0, 1], np.int32)))


# ---------------------------------------------------------------- per-cluster factors
def mixed_sizes_input():
    """Six parents with 2, 4, 0, 18, 130 and 512 users; usersPerSubCluster = 2 makes k_c = 1, 2, -, 9, 65, 256."""
    rng = np.random.default_rng(77)
    sizes = [2, 4, 0, 18, 130, 512]
    n_users, n_items = sum(sizes), 150
    A = (rng.random((n_users, n_items)) < 0.15) * rng.integers(1, 6, (n_users, n_items))
    A[np.arange(n_users), rng.integers(0, n_items, n_users)] = 3          # every user rates something
    u, i = np.nonzero(A)
    s = A[u, i].astype(np.float32)
    u, i, s = np.r_[u + 1, [1, 2]], np.r_[i + 1, [1, 1]], np.r_[s, np.float32([0.0, -1.0])]     # dropped by score > 0
    order = rng.permutation(len(u))
    users = rng.permutation(n_users) + 1
    cl = np.repeat(np.arange(len(sizes)), sizes)
    return (u[order].astype(np.int32), i[order].astype(np.int32), s[order].astype(np.float32)), users.astype(np.int32), cl.astype(np.int32), len(sizes)


@pytest.mark.parametrize("ppc", [False, True])
@pytest.mark.parametrize("norm", [0, -1, 2])
def test_factors_match_the_oracle_per_parent(ctx, ppc, norm):
    P = pkg()
    (u, i, s), mu, mc, K = mixed_sizes_input()
    ups, iters = 2, 3
    m = RR.mappings(u, i, s, mu, mc, K)
    kc = RR.sub_clusters(m, ups)
    assert kc == [1, 2, 0, 9, 65, 256]
    rng = np.random.default_rng(5)
    H0 = [rng.random((len(m["users"][c]), kc[c])) + 0.01 for c in range(K)]
    W0 = [rng.random((len(m["items"][c]), kc[c])) + 0.01 for c in range(K)]
    job = P.ClusterRefinementJob(conf_of(numberOfUsers=len(mu), numberOfClusters=K, usersPerSubCluster=ups, numberOfIterations=iters,
                                         normalizationFrequency=norm), ctx, ppc=ppc)
    users, clusters, counts = job.run((u, i, s), (mu, mc), H0=H0, W0=W0, keep_factors=True)
    assert job.sub_clusters.tolist() == kc and job.users_in_cluster.tolist() == [len(x) for x in m["users"]]
    assert job.stats["sum_k"] == sum(kc) and job.stats["sum_users"] == len(mu) and job.stats["nnz"] == int(m["kept"].sum())
    for c in range(K):
        H, W = job.factors[c]
        if kc[c] == 0:
            assert H.size == 0 and W.size == 0
            continue
        su, si, ss = RR.extract(u, i, s, m, c)
        Ho, Wo = oracle.nmf(su, si, ss, H0[c], W0[c], iterations=iters, ppc=ppc, normalization_frequency=norm)
        print("parent %d k %d: worst relative error H %.3e W %.3e" % (c, kc[c], np.max(np.abs(H - Ho) / np.abs(Ho)), np.max(np.abs(W - Wo) / np.abs(Wo))))
        np.testing.assert_allclose(H, Ho, rtol=1e-10, atol=1e-300)
        np.testing.assert_allclose(W, Wo, rtol=1e-10, atol=1e-300)
        if ppc and norm == -1:
            np.testing.assert_allclose(np.abs(H).sum(1), 1.0, rtol=1e-12)
    # the clustering of the same call: argmax of these rows with the parent's offset
    stride = -(-len(mu) // K)
    want = np.concatenate([c * stride + job.factors[c][0].argmax(1) for c in range(K) if kc[c]])
    assert users.tolist() == np.concatenate(m["users"]).tolist() and clusters.tolist() == want.tolist()
    assert counts.sum() == len(mu) and np.array_equal(np.bincount(clusters, minlength=len(counts)), counts)


def assert_parents_match_the_oracle(job, coo, m, kc, H0, W0, iters, ppc, norm, label):
    u, i, s = coo
    for c in range(len(kc)):
        H, W = job.factors[c]
        su, si, ss = RR.extract(u, i, s, m, c)
        Ho, Wo = oracle.nmf(su, si, ss, H0[c], W0[c], iterations=iters, ppc=ppc, normalization_frequency=norm)
        assert np.isfinite(Ho).all() and np.isfinite(Wo).all()
        print("%s parent %d k %d: worst relative error H %.3e W %.3e" % (label, c, kc[c], FE.worst_relative(H, Ho), FE.worst_relative(W, Wo)))
        np.testing.assert_allclose(H, Ho, rtol=1e-10, atol=1e-300, err_msg="H of parent %d" % c)
        np.testing.assert_allclose(W, Wo, rtol=1e-10, atol=1e-300, err_msg="W of parent %d" % c)


@pytest.mark.parametrize("ups", [8, 120])
@pytest.mark.parametrize("ppc", [False, True])
@pytest.mark.parametrize("norm", [0, 2])
def test_long_rows_per_parent_vs_oracle(ctx, ups, ppc, norm):
    """FE.parents: user and item rows of several chunks inside a parent.  usersPerSubCluster = 8 puts the 600-user parent (items
    with 257, 515 and 600 raters, a user with 700 ratings) into the k > 64 branch and the users with 255 .. 513 ratings into a
    k = 5 parent; 120 puts the 600-user parent's long item rows into the k <= 64 branch (an item row cannot be longer than its
    parent has users, and 8 users per sub-cluster with k <= 64 allow 512)."""
    P = pkg()
    d = FE.parents()
    u, i, s = d["coo"]
    mu, mc, K, iters = d["map_user"], d["map_cluster"], d["K"], 3
    m = RR.mappings(u, i, s, mu, mc, K)
    kc = RR.sub_clusters(m, ups)
    assert kc == ([75, 5, 1] if ups == 8 else [5, 1, 1])
    rng = np.random.default_rng(600 + ups)
    H0 = [rng.random((len(m["users"][c]), kc[c])) + 0.01 for c in range(K)]
    W0 = [rng.random((len(m["items"][c]), kc[c])) + 0.01 for c in range(K)]
    job = P.ClusterRefinementJob(conf_of(numberOfUsers=d["n_users"], numberOfClusters=K, usersPerSubCluster=ups, numberOfIterations=iters,
                                         normalizationFrequency=norm), ctx, ppc=ppc)
    users, clusters, counts = job.run((u, i, s), (mu, mc), H0=H0, W0=W0, keep_factors=True)
    assert job.sub_clusters.tolist() == kc and job.stats["nnz"] == int(m["kept"].sum()) == len(u) - 2
    assert_parents_match_the_oracle(job, (u, i, s), m, kc, H0, W0, iters, ppc, norm, "ups %d" % ups)
    stride = -(-d["n_users"] // K)
    want = np.concatenate([c * stride + job.factors[c][0].argmax(1) for c in range(K)])
    assert users.tolist() == np.concatenate(m["users"]).tolist() and clusters.tolist() == want.tolist()
    assert counts.sum() == d["n_users"] and np.array_equal(np.bincount(clusters, minlength=len(counts)), counts)
    assert job.stats["collisions"] == 0


@pytest.mark.parametrize("ppc", [True, False])
def test_wave_loops_wrap(ctx, ppc):
    """FE.wrap as one parent of 17 000 users with 400 users per sub-cluster: k = 43, so a wave serves one row and the loops over
    user rows and user chunks by wave (k_rf_init, k_rf_spmm, k_rf_update) go round more than once, as do the passes over the
    1.05 M ratings (k_rf_item_presence, k_rf_keys).  The thread-per-row loops of the mappings and of k_rf_assign wrap only above
    1 048 576 rows and are not compared at such a size."""
    P = pkg()
    (u, i, s), mu, mc = FE.wrap_as_one_parent()
    ups, iters, seed = FE.WRAP_USERS_PER_SUB_CLUSTER, 2, 31
    m = RR.mappings(u, i, s, mu, mc, 1)
    kc = RR.sub_clusters(m, ups)
    assert kc == [43]
    H0, W0 = RR.seeded_initial(m, kc, seed)
    job = P.ClusterRefinementJob(conf_of(numberOfUsers=len(mu), numberOfClusters=1, usersPerSubCluster=ups, numberOfIterations=iters,
                                         normalizationFrequency=2), ctx, ppc=ppc)
    users, clusters, counts = job.run((u, i, s), (mu, mc), seed=seed, keep_factors=True)
    H, W = job.factors[0]
    assert H.shape == H0[0].shape and W.shape == W0[0].shape
    assert not (H == H0[0]).all(1).any() and not (W == W0[0]).all(1).any()      # a row the wrapped loop passed over keeps its initial value
    assert_parents_match_the_oracle(job, (u, i, s), m, kc, H0, W0, iters, ppc, 2, "wrap")
    assert users.tolist() == mu.tolist() and clusters.tolist() == H.argmax(1).tolist() and counts.sum() == len(mu)


@pytest.mark.parametrize("ppc", [True, False])
@pytest.mark.parametrize("iters", [1, 2])
def test_infinities_are_clamped_like_the_reference(ctx, ppc, iters):
    """Initial matrices around 1e200 (test_nmf_gpu.py has the reasoning): every parent's factors stay finite and equal the
    oracle's, which clamps an infinite sum to Double.MAX_VALUE like the reference."""
    P = pkg()
    u, i, s, users = small_input()
    mc = (users % 2).astype(np.int32)
    ups = 5
    m = RR.mappings(u, i, s, users, mc, 2)
    kc = RR.sub_clusters(m, ups)
    assert kc == [4, 4]
    rng = np.random.default_rng(200)
    H0 = [FE.huge_initial(rng, (len(m["users"][c]), kc[c])) for c in range(2)]
    W0 = [FE.huge_initial(rng, (len(m["items"][c]), kc[c])) for c in range(2)]
    for c in range(2):
        with np.errstate(over="ignore"):
            assert np.isinf(W0[c].T @ W0[c]).all() and np.isinf(H0[c].T @ H0[c]).all()
        if ppc:                                           # the case does need the clamp: without it, inf / inf
            assert np.isnan(FE.unclamped_ppc_row(*RR.extract(u, i, s, m, c), H0[c], W0[c], 0)).all()
    job = P.ClusterRefinementJob(conf_of(numberOfUsers=len(users), numberOfClusters=2, usersPerSubCluster=ups, numberOfIterations=iters,
                                         normalizationFrequency=0), ctx, ppc=ppc)
    job.run((u, i, s), (users, mc), H0=H0, W0=W0, keep_factors=True)
    for H, W in job.factors:
        assert np.isfinite(H).all() and np.isfinite(W).all()
    assert_parents_match_the_oracle(job, (u, i, s), m, kc, H0, W0, iters, ppc, 0, "clamp")


# ---------------------------------------------------------------- refined clustering
@pytest.mark.parametrize("seed", RR.ml100k_case()["seeds"])
def test_refined_clustering_matches_the_composed_oracles(ctx, seed):
    """The device draws the initial matrices from the seed; the oracles start from the numpy restatement of the same formula."""
    P = pkg()
    case = RR.ml100k_case()
    u, i, s = case["coo"]
    m = RR.mappings(u, i, s, case["map_user"], case["map_cluster"], case["K"])
    kc = RR.sub_clusters(m, case["users_per_sub_cluster"])
    H0, W0 = RR.seeded_initial(m, kc, seed)
    ou, oc, ocount, _, ties, _ = RR.composed_refinement(u, i, s, case["map_user"], case["map_cluster"], case["K"], case["users_per_sub_cluster"],
                                                        case["n_users"], case["iterations"], True, case["normalization_frequency"], H0, W0)
    job = P.ClusterRefinementJob(conf_of(numberOfUsers=case["n_users"], numberOfClusters=case["K"], usersPerSubCluster=case["users_per_sub_cluster"],
                                         numberOfIterations=case["iterations"], normalizationFrequency=case["normalization_frequency"]), ctx)
    users, clusters, counts = job.run((u, i, s), (case["map_user"], case["map_cluster"]), seed=seed)
    assert users.tolist() == ou.tolist()
    differ = clusters != oc
    print("seed %d: %d users differ, %d near-ties, launches %d, iterations %.3f ms" % (seed, differ.sum(), ties.sum(), job.stats["launches"], job.stats["ms_iterations"]))
    assert ties.sum() <= 0.001 * len(users)
    assert not (differ & ~ties).any(), np.flatnonzero(differ & ~ties)[:10]
    assert counts.sum() == len(case["map_user"])
    assert np.array_equal(np.bincount(clusters, minlength=len(counts)), counts)
    if not differ.any():
        assert np.array_equal(counts, ocount)
    assert job.stats["collisions"] == 0
    assert job.stats["launches"] <= 40 + 8 * case["iterations"]        # one launch set per iteration, not one per parent


# ---------------------------------------------------------------- errors
def small_input():
    rng = np.random.default_rng(3)
    n_users, n_items = 40, 25
    A = (rng.random((n_users, n_items)) < 0.3) * rng.integers(1, 6, (n_users, n_items))
    A[np.arange(n_users), rng.integers(0, n_items, n_users)] = 2
    u, i = np.nonzero(A)
    return (u + 1).astype(np.int32), (i + 1).astype(np.int32), A[u, i].astype(np.float32), np.arange(1, n_users + 1, dtype=np.int32)


def test_errors_mirror_the_reference(ctx):
    P = pkg()
    u, i, s, users = small_input()
    cl = (users % 2).astype(np.int32)
    conf = conf_of(numberOfUsers=60, numberOfClusters=2, usersPerSubCluster=5, numberOfIterations=2)
    # user 57 is in the map (parent 1) and rated nothing; user 8's only ratings are <= 0
    with pytest.raises(RuntimeError, match=r"User 57 has not rated any item \(parent cluster 1\)"):
        P.ClusterRefinementJob(conf, ctx).run((u, i, s), (np.r_[users, 57].astype(np.int32), np.r_[cl, 1].astype(np.int32)))
    s8 = np.where(u == 8, np.float32(-1.0), s).astype(np.float32)
    with pytest.raises(RuntimeError, match=r"User 8 has not rated any item \(parent cluster 0\)"):
        P.ClusterRefinementJob(conf, ctx).run((u, i, s8), (users, cl))
    # item 31 is rated only by user 44, whom the map does not name: it joins parent 0's items and nobody of parent 0 rated it
    u2, i2, s2 = np.r_[u, 44].astype(np.int32), np.r_[i, 31].astype(np.int32), np.r_[s, 4.0].astype(np.float32)
    with pytest.raises(RuntimeError, match=r"Item 31 has not been rated by anybody \(parent cluster 0\)"):
        P.ClusterRefinementJob(conf, ctx).run((u2, i2, s2), (users, cl))
    # with no iteration asked for nothing is factorised and nothing fails
    users0, _, counts0 = P.ClusterRefinementJob(conf_of(numberOfUsers=60, numberOfClusters=2, usersPerSubCluster=5, numberOfIterations=0), ctx).run((u2, i2, s2), (users, cl))
    assert len(users0) == 40 and counts0.sum() == 40


def test_more_than_256_sub_clusters_are_rejected(ctx):
    P = pkg()
    n = 300
    users = np.arange(1, n + 1, dtype=np.int32)
    cl = np.where(users <= 258, 1, 0).astype(np.int32)
    conf = conf_of(numberOfUsers=n, numberOfClusters=2, usersPerSubCluster=1, numberOfIterations=1)
    with pytest.raises(RuntimeError, match=r"parent cluster 1: 258 users .* exceed the kernel limit 256"):
        P.ClusterRefinementJob(conf, ctx).run((users, np.ones(n, np.int32), np.ones(n, np.float32)), (users, cl))
    cl = np.where(users <= 256, 1, 0).astype(np.int32)              # 256 is still served
    _, clusters, counts = P.ClusterRefinementJob(conf, ctx).run((users, np.ones(n, np.int32), np.ones(n, np.float32)), (users, cl))
    assert counts.sum() == n


def test_colliding_ids_are_counted_not_hidden(ctx):
    """numberOfUsers = 4 with two parents makes the id stride 2, parent 0 has 20 users in 4 sub-clusters: a user of parent 0 whose
    argmax is 2 or 3 gets an id of parent 1's range, as in the reference."""
    P = pkg()
    u, i, s, users = small_input()
    cl = (users > 20).astype(np.int32)
    job = P.ClusterRefinementJob(conf_of(numberOfUsers=4, numberOfClusters=2, usersPerSubCluster=5, numberOfIterations=4), ctx)
    got_users, clusters, counts = job.run((u, i, s), (users, cl), seed=9, keep_factors=True)
    assert job.sub_clusters.tolist() == [4, 4]
    arg = np.concatenate([job.factors[c][0].argmax(1) for c in range(2)])
    assert clusters.tolist() == (np.repeat([0, 1], 20) * 2 + arg).tolist()
    assert job.stats["collisions"] == int((arg >= 2).sum()) > 0
    assert len(counts) == 1 * 2 + 4 and counts.sum() == 40          # the last parent's ids run past numberOfClusters x stride
    assert np.array_equal(np.bincount(clusters, minlength=len(counts)), counts)


# ---------------------------------------------------------------- determinism and the device's generator
def test_same_seed_same_bits(ctx):
    P = pkg()
    (u, i, s), mu, mc, K = mixed_sizes_input()
    conf = conf_of(numberOfUsers=len(mu), numberOfClusters=K, usersPerSubCluster=8, numberOfIterations=5, normalizationFrequency=2)
    runs = []
    for seed in (21, 21, 22):
        job = P.ClusterRefinementJob(conf, ctx)
        out = job.run((u, i, s), (mu, mc), seed=seed, keep_factors=True)
        runs.append((out, job.factors))
    (a, fa), (b, fb), (c, fc) = runs
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for (ha, wa), (hb, wb) in zip(fa, fb):
        assert ha.tobytes() == hb.tobytes() and wa.tobytes() == wb.tobytes()
    assert any(ha.tobytes() != hc.tobytes() for (ha, _), (hc, _) in zip(fa, fc))
    # no iteration: the factors are the initial matrices, bit for bit the header's formula
    job = P.ClusterRefinementJob(conf_of(numberOfUsers=len(mu), numberOfClusters=K, usersPerSubCluster=8, numberOfIterations=0), ctx)
    job.run((u, i, s), (mu, mc), seed=2 ** 63 + 12345, keep_factors=True)
    for c in range(K):
        H, W = job.factors[c]
        assert np.array_equal(H, RR.initial_matrix(2 ** 63 + 12345, c, 0, *H.shape)) and np.array_equal(W, RR.initial_matrix(2 ** 63 + 12345, c, 1, *W.shape))


# ---------------------------------------------------------------- the driver
def test_driver_runs_the_whole_pipeline(ctx):
    P = pkg()
    case = RR.ml100k_case()
    u, i, s = case["coo"]
    top_n = 10
    conf = conf_of(numberOfUsers=case["n_users"], numberOfItems=case["n_items"], numberOfClusters=case["K"],
                   usersPerSubCluster=case["users_per_sub_cluster"], numberOfRecommendations=top_n)
    R = P.Ratings(ctx, u, i, s)
    try:
        driver = P.RMRecommenderDriver(conf, ctx)
        rec, (users, clusters, counts) = driver.run(R, seed=4)
        rows = rec.rows()
        stride = -(-case["n_users"] // case["K"])
        assert len(counts) == case["K"] * stride and counts.sum() == case["n_users"] == len(users)
        assert len(np.unique(clusters)) > case["K"] and driver.stats["refine"]["collisions"] == 0
        assert set(driver.stats) == {"ppc", "refine", "rm2"}
        print("driver: ppc %.2f ms, refine %.2f ms (%d launches), rm2 %.2f ms" % (driver.stats["ppc"]["ms_total"], driver.stats["refine"]["ms_total"],
                                                                                 driver.stats["refine"]["launches"], driver.stats["rm2"]["ms_total"]))
        # the same rows as the RM2 job fed with the returned clustering: the long, sparse counts array is accepted as it is
        rm2_conf = conf_of(numberOfItems=case["n_items"], numberOfClusters=len(counts), numberOfRecommendations=top_n)
        again = P.RM2Job(rm2_conf, ctx).run(R, clustering=(users, clusters), clustering_count=counts).rows()
        for k in ("user", "item", "score", "cluster"):
            assert np.array_equal(rows[k], again[k]), k
        ref = oracle.rm2(u, i, s, lam=0.1, number_of_items=case["n_items"], number_of_recommendations=1 << 30, number_of_clusters=len(counts),
                         map_user=users, map_cluster=clusters, cluster_count=counts, n_threads=8)
        assert_topn_matches(rows, ref, top_n)                # purely relative, 1e-5
        # numberOfRecommendations = 0 stops in front of the RM2 job, with the same clustering
        conf0 = P.Configuration(conf)
        conf0.setInt("numberOfRecommendations", 0)
        d0 = P.RMRecommenderDriver(conf0, ctx)
        rec0, (users0, clusters0, counts0) = d0.run(R, seed=4)
        assert rec0 is None and "rm2" not in d0.stats
        assert np.array_equal(users0, users) and np.array_equal(clusters0, clusters) and np.array_equal(counts0, counts)
        # numberOfIterations = 0 takes the caller's clustering: no factorisation, no refinement
        conf1 = P.Configuration(conf)
        conf1.setInt("numberOfIterations", 0)
        conf1.setInt("numberOfClusters", len(counts))
        d1 = P.RMRecommenderDriver(conf1, ctx)
        rec1, (users1, clusters1, counts1) = d1.run(R, clustering=(users, clusters), clustering_count=counts)
        assert set(d1.stats) == {"rm2"} and np.array_equal(clusters1, clusters)
        rows1 = rec1.rows()
        for k in ("user", "item", "score", "cluster"):
            assert np.array_equal(rows[k], rows1[k]), k
    finally:
        R.close()


def assert_ppc_stage_matches(got, want):
    """Tie-tolerant, as test_refined_clustering_matches_the_composed_oracles compares."""
    (users, clusters, counts), (ou, oc, ocount, ties) = got, want
    assert users.tolist() == ou.tolist()
    differ = clusters != oc
    print("driver ppc stage: %d users differ, %d near-ties" % (differ.sum(), ties.sum()))
    assert ties.sum() <= 0.001 * len(users)
    assert not (differ & ~ties).any(), np.flatnonzero(differ & ~ties)[:10]
    assert counts.sum() == len(users) and np.array_equal(np.bincount(clusters, minlength=len(counts)), counts)
    if not differ.any():
        assert np.array_equal(counts, ocount)


def test_driver_ppc_stage_matches_the_oracle(ctx):
    """The clustering the driver's first stage hands on (ten PPC iterations from the seeded draw, normalizationFrequency 12, then
    the argmax) against oracle.nmf and oracle.cluster_assign from the restated draw.  A user whose two largest oracle entries
    differ by no more than 1e-8 relative may differ, at most 0.1 % of the users: with 943 users that admits nobody, and the
    oracle alone has 0 near-ties for seed 4 (test_refine_cpu.py checks that without a GPU)."""
    P = pkg()
    case = RR.ml100k_case()
    seed = RR.DRIVER_PPC_SEED
    ou, oc, ocount, ties, H0, W0 = RR.driver_ppc_stage(case, seed)
    conf = conf_of(numberOfUsers=case["n_users"], numberOfItems=case["n_items"], numberOfClusters=case["K"], usersPerSubCluster=-1,
                   numberOfRecommendations=0)
    R = P.Ratings(ctx, *case["coo"])
    try:
        driver = P.RMRecommenderDriver(conf, ctx)
        rec, got = driver.run(R, seed=seed)
        assert rec is None and set(driver.stats) == {"ppc"}
        assert_ppc_stage_matches(got, (ou, oc, ocount, ties))
        # the caller's matrices instead of the seed's
        rec, again = P.RMRecommenderDriver(conf, ctx).run(R, H=H0, W=W0, seed=seed + 1)
        assert rec is None
        assert_ppc_stage_matches(again, (ou, oc, ocount, ties))
    finally:
        R.close()
