"""Cluster refinement without a GPU: the ABI's new structs, the argument checks in front of the device, the numpy restatement of
the seed generator, and the oracle-only half of the refined-clustering check (the seeds test_refine_gpu.py uses stay within the
cap of users excused by near-ties)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import refine_ref as RR
from util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoDevice:
    """A context whose handle must never reach the library."""

    @property
    def _h(self):
        raise AssertionError("the device was touched")


def _struct_body(name):
    header = open(os.path.join(ROOT, "include", "filmyou.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(typ, n.strip()) for n in names.split(",")]
    return fields


def test_struct_sizes_match_the_header():
    P = pkg()
    size = {"int32_t": 4, "uint32_t": 4, "int64_t": 8, "uint64_t": 8, "double": 8}
    for name, struct in (("fy_refine_params", P._native.RefineParams), ("fy_refine_stats", P._native.RefineStats)):
        fields = _struct_body(name)
        assert [n for _, n in fields] == [n for n, _ in struct._fields_]
        assert [size[t] for t, _ in fields] == [C.sizeof(t) for _, t in struct._fields_]
    assert C.sizeof(P._native.RefineParams) == 32           # six int32, one uint64: no padding
    assert C.sizeof(P._native.RefineStats) == 10 * 8
    assert C.sizeof(P._native.Stats) == 33 * 8 and P._native.load().fy_abi_version() == 5      # the old ABI is untouched


def test_native_argument_checks_fire_before_the_device_is_touched():
    P = pkg()
    P.build()
    lib = P._native.load()
    out = C.c_void_p()
    ok = P._native.RefineParams(10, 2, 5, 1, 1, -1, 0)
    one = np.ones(1, np.int32)
    fake = C.c_void_p(1)            # a non-NULL context / ratings handle: a check that let it through would crash
    assert lib.fy_cluster_refine(None, C.byref(ok), None, 0, None, None, None, None, None) == -1
    assert b"out is NULL" in lib.fy_last_error()
    assert lib.fy_cluster_refine(None, None, None, 0, None, None, None, None, C.byref(out)) == -1
    assert b"params is NULL" in lib.fy_last_error()
    for field, value, word in (("users_per_sub_cluster", 0, b"usersPerSubCluster"), ("users_per_sub_cluster", -1, b"usersPerSubCluster"),
                               ("number_of_clusters", 0, b"Invalid number of clusters"), ("number_of_clusters", -3, b"Invalid number of clusters")):
        bad = P._native.RefineParams(10, 2, 5, 1, 1, -1, 0)
        setattr(bad, field, value)
        assert lib.fy_cluster_refine(fake, C.byref(bad), fake, 0, None, None, None, None, C.byref(out)) == -1
        assert word in lib.fy_last_error(), lib.fy_last_error()
    assert lib.fy_cluster_refine(fake, C.byref(ok), fake, 1, None, None, None, None, C.byref(out)) == -1      # n_map > 0, NULL map
    assert lib.fy_cluster_refine(fake, C.byref(ok), fake, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, None, C.byref(out)) == -1
    assert b"H0 and W0" in lib.fy_last_error()
    assert lib.fy_cluster_refine(None, C.byref(ok), None, 0, None, None, None, None, C.byref(out)) == -1
    assert b"NULL" in lib.fy_last_error()
    assert lib.fy_submap_create(fake, fake, 0, 0, None, None, C.byref(out)) == -1
    assert b"Invalid number of clusters" in lib.fy_last_error()
    assert lib.fy_submap_create(None, None, 2, 0, None, None, C.byref(out)) == -1
    assert lib.fy_submap_create(fake, fake, 2, 0, None, None, None) == -1
    assert lib.fy_refined_n_users(None) == 0 and lib.fy_submap_n_users(None) == 0
    lib.fy_refined_free(None)
    lib.fy_submap_destroy(None)


def test_host_argument_checks_fire_before_the_device_is_touched():
    P = pkg()
    u = np.array([1], np.int32)
    ratings = (u, u, np.ones(1, np.float32))

    def conf(**kw):
        c = P.Configuration()
        for k, v in kw.items():
            c.setInt(k, v)
        return c
    with pytest.raises(ValueError, match="usersPerSubCluster must be > 0"):
        P.ClusterRefinementJob(conf(numberOfUsers=4, numberOfClusters=2, usersPerSubCluster=0), _NoDevice()).run(ratings, (u, u))
    with pytest.raises(ValueError, match="usersPerSubCluster must be > 0"):
        P.ClusterRefinementJob(conf(numberOfUsers=4, numberOfClusters=2), _NoDevice()).run(ratings, (u, u))
    with pytest.raises(ValueError, match="Invalid number of clusters"):
        P.ClusterRefinementJob(conf(numberOfUsers=4, numberOfClusters=0, usersPerSubCluster=2), _NoDevice()).run(ratings, (u, u))
    with pytest.raises(ValueError, match="Invalid number of clusters"):
        P.SubClusterMappingJob(conf(), _NoDevice()).run(ratings, (u, u))
    with pytest.raises(ValueError, match="differ in length"):
        P.SubClusterMappingJob(conf(numberOfClusters=2), _NoDevice()).run(ratings, (u, np.r_[u, u]))
    with pytest.raises(ValueError, match="given together"):
        P.ClusterRefinementJob(conf(numberOfUsers=4, numberOfClusters=2, usersPerSubCluster=2), _NoDevice()).run(ratings, (u, u), H0=[np.ones((1, 1))])
    with pytest.raises(ValueError, match="are required"):
        P.RMRecommenderDriver(conf(numberOfUsers=4, numberOfItems=3), _NoDevice()).run(ratings)
    with pytest.raises(ValueError, match="needs the caller's clustering"):
        P.RMRecommenderDriver(conf(numberOfUsers=4, numberOfItems=3, numberOfClusters=2, numberOfIterations=0), _NoDevice()).run(ratings)


def test_the_driver_leaves_the_shared_defaults_alone():
    P = pkg()
    assert "numberOfIterations" not in P.Configuration.DEFAULTS and "normalizationFrequency" not in P.Configuration.DEFAULTS
    assert "usersPerSubCluster" not in P.Configuration.DEFAULTS
    c = P.Configuration()
    c.setInt("numberOfClusters", 3)
    staged = P.RMRecommenderDriver(c)._stage_conf()
    assert staged.getInt("numberOfIterations", -7) == 10 and staged.getInt("normalizationFrequency", -7) == 12      # RMRecommenderDriver.java:94, 115
    assert staged.getInt("usersPerSubCluster", -7) == -1 and staged.getInt("numberOfRecommendations", -7) == 1000
    assert "numberOfIterations" not in c                                        # the caller's object is not written to


def test_seed_generator_restatement():
    # splitmix64's published first outputs from state 0 are mix(0), mix(golden), ...: the step function is the textbook one
    assert int(RR.mix(np.uint64(0))) == 0xE220A8397B1DCDAF
    assert int(RR.mix(np.uint64(0x9E3779B97F4A7C15))) == 0x6E789E6AA1B965F4
    A = RR.initial_matrix(5, 3, 0, 40, 7)
    assert A.shape == (40, 7) and A.dtype == np.float64
    assert (A > 0).all() and (A <= 1).all()
    # one element at a time, in Python integers
    M = (1 << 64) - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)
    for seed, c, which, r, k in ((5, 3, 0, 39, 6), (2 ** 63 + 9, 49, 1, 0, 0), (0, 0, 0, 1, 1)):
        z = mix(seed ^ mix(((c << 32) | which) ^ mix((r << 32) | k)))
        want = ((z >> 11) + 1) * 2.0 ** -53
        assert RR.initial_matrix(seed, c, which, r + 1, k + 1)[r, k] == want
    # a counter-based formula: a larger matrix starts with the smaller one; seed, cluster and matrix all matter
    assert np.array_equal(RR.initial_matrix(5, 3, 0, 50, 9)[:40, :7], A)
    for other in (RR.initial_matrix(6, 3, 0, 40, 7), RR.initial_matrix(5, 4, 0, 40, 7), RR.initial_matrix(5, 3, 1, 40, 7)):
        assert not np.array_equal(other, A)
    big = RR.initial_matrix(1, 0, 0, 400, 50)
    assert abs(big.mean() - 0.5) < 0.01 and len(np.unique(big)) == big.size


def test_mappings_restatement_on_a_hand_example():
    # users 1, 2 in cluster 1, user 3 in cluster 0, user 9 mapped (cluster 0) without any rating, user 4 not in the map
    u = np.array([1, 1, 2, 3, 4, 4, 2])
    i = np.array([5, 6, 6, 7, 8, 5, 9])
    s = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 0.0, -1.0])
    m = RR.mappings(u, i, s, [1, 2, 3, 9, 2], [0, 0, 0, 0, 1], 2)       # user 2 appears twice, the later entry wins; user 1 -> 0
    assert [x.tolist() for x in m["users"]] == [[1, 3, 9], [2]]
    assert [x.tolist() for x in m["items"]] == [[5, 6, 7, 8], [6]]        # item 8 through the unmapped user 4; item 9 has score <= 0
    assert m["kept"].tolist() == [True, True, True, True, False, False, False]
    assert m["row_user"].tolist() == [0, 0, 3, 1] and m["row_item"].tolist() == [0, 1, 4, 2]


def test_oracle_alone_stays_within_the_near_tie_cap():
    """test_refine_gpu.py excuses users whose two largest oracle H entries differ by no more than 1e-8 relative, at most 0.1 %
    of them: the seeds it uses must leave the oracle's own result inside that cap."""
    case = RR.ml100k_case()
    u, i, s = case["coo"]
    m = RR.mappings(u, i, s, case["map_user"], case["map_cluster"], case["K"])
    kc = RR.sub_clusters(m, case["users_per_sub_cluster"])
    assert sum(len(x) for x in m["users"]) == case["n_users"] and min(kc) >= 2
    for seed in case["seeds"]:
        H0, W0 = RR.seeded_initial(m, kc, seed)
        users, clusters, counts, _, ties, _ = RR.composed_refinement(u, i, s, case["map_user"], case["map_cluster"], case["K"],
                                                                      case["users_per_sub_cluster"], case["n_users"], case["iterations"], True,
                                                                      case["normalization_frequency"], H0, W0)
        assert counts.sum() == case["n_users"] == len(users)
        assert ties.sum() <= 0.001 * len(users), (seed, int(ties.sum()))
        assert len(np.unique(clusters)) > case["K"]              # the sub-runs really split their parents


def test_oracle_alone_leaves_the_driver_ppc_stage_without_near_ties():
    """test_driver_ppc_stage_matches_the_oracle excuses near-tie users under the same cap; with the ML-100K case's 943 users the cap
    admits none, and seed 4 has none."""
    case = RR.ml100k_case()
    users, clusters, counts, ties, _, _ = RR.driver_ppc_stage(case, RR.DRIVER_PPC_SEED)
    assert len(users) == case["n_users"] == counts.sum()
    assert ties.sum() <= 0.001 * len(users), int(ties.sum())
    assert (counts > 0).all()                                    # the PPC stage uses every cluster
