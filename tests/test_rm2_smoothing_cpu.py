"""Dirichlet-prior and absolute-discounting smoothing beside Jelinek-Mercer: the plain statement of the three methods
(tests/rm2_smoothing_definition.py) is pinned to the reference's estimator through oracle.rm2, the two identities that tie the new
methods to it hold on the CPU, and the host maps the Configuration keys.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle
from rm2_smoothing_definition import definition_full, definition_rows
from util import pkg, synth

ULP32 = 2.0 ** -23      # the oracle emits (float) scores: two fp64 evaluations of one score differ by at most one float rounding


def by_pair(ref):
    return {(int(a), int(b)): (float(c), int(d)) for a, b, c, d in zip(ref["rec_user"], ref["rec_item"], ref["rec_score"], ref["rec_cluster"])}


def assert_same_scores(got, want, rel):
    """same (user, item) rows, same clusters, same -inf pattern, finite scores within `rel`; returns the worst relative difference"""
    g, w = by_pair(got), by_pair(want)
    assert g.keys() == w.keys()
    worst = 0.0
    for k, (sw, cw) in w.items():
        sg, cg = g[k]
        assert cg == cw
        if np.isfinite(sw):
            worst = max(worst, abs(sg - sw) / abs(sw))
        else:
            assert sg == sw, k
    assert worst <= rel, worst
    return worst


def equal_sum_data(n_users, n_items, seed=5):
    """identity 1: every user rates 5 distinct items with a permutation of {0.5, 1, 2, 3.5, 5}: every rating sum is 12"""
    rng = np.random.default_rng(seed)
    vals = np.array([0.5, 1.0, 2.0, 3.5, 5.0], dtype=np.float32)
    u = np.repeat(np.arange(1, n_users + 1, dtype=np.int32), 5)
    i = np.concatenate([rng.choice(n_items, size=5, replace=False) + 1 for _ in range(n_users)]).astype(np.int32)
    s = np.concatenate([rng.permutation(vals) for _ in range(n_users)]).astype(np.float32)
    return u, i, s, 12.0


def equal_rating_data(n_users, n_items, r0=3.0, seed=6):
    """identity 2: every rating equals r0; between 2 and 9 ratings per user"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(2, 10, size=n_users)
    u = np.repeat(np.arange(1, n_users + 1, dtype=np.int32), deg)
    i = np.concatenate([rng.choice(n_items, size=int(d), replace=False) + 1 for d in deg]).astype(np.int32)
    s = np.full(len(u), r0, dtype=np.float32)
    return u, i, s, r0


def test_jm_definition_is_the_oracle_on_the_golden_fixture(rm_golden):
    g = rm_golden
    u, i, s = g["coo"]
    ref = oracle.rm2(u, i, s, lam=0.5, number_of_items=g["numberOfItems"], number_of_recommendations=1 << 30,
                     number_of_clusters=g["numberOfClusters"], map_user=g["map_user"], map_cluster=g["map_cluster"])
    got = definition_full(u, i, s, "jm", 0.5, g["numberOfItems"], clustering=(g["map_user"], g["map_cluster"]))
    assert len(got["rec_user"]) == len(ref["rec_user"]) == 507
    print("golden fixture, worst relative difference %.2e" % assert_same_scores(got, ref, ULP32))


@pytest.mark.parametrize("K,lam", [(1, 0.1), (7, 0.1), (7, 0.0)])
def test_jm_definition_is_the_oracle_on_the_tiny_shape(K, lam):
    S = synth()
    u, i, s, facts = S.generate("tiny")
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    uu = np.unique(u)
    mc = S.hash_clustering(uu, K)
    ref = oracle.rm2(u, i, s, lam=lam, number_of_items=facts["n_items"], number_of_recommendations=1 << 30, number_of_clusters=K,
                     map_user=uu, map_cluster=mc)
    got = definition_full(u, i, s, "jm", lam, facts["n_items"], clustering=(uu, mc))
    print("tiny, %d clusters, lambda %g: worst relative difference %.2e" % (K, lam, assert_same_scores(got, ref, ULP32)))


@pytest.mark.parametrize("method,param", [("jm", 0.1), ("dirichlet", 50.0), ("dirichlet", 0.0), ("absoluteDiscounting", 1.0)])
def test_rows_definition_equals_the_dense_definition(method, param):
    """the rows-only evaluator (the three-term identity) against the dense statement, 7 clusters of the tiny shape, every candidate"""
    S = synth()
    u, i, s, facts = S.generate("tiny")
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    uu = np.unique(u)
    mc = S.hash_clustering(uu, 7)
    full = definition_full(u, i, s, method, param, facts["n_items"], clustering=(uu, mc), score_dtype=np.float64)
    rows = {"user": full["rec_user"], "item": full["rec_item"], "cluster": full["rec_cluster"]}
    got = definition_rows((u, i, s), rows, method, param, facts["n_items"], clustering=(uu, mc))
    want = full["rec_score"]
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin])
    worst = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin])))
    print("%s %g: %d rows, %d of them -inf, worst relative difference %.2e" % (method, param, len(want), int((~fin).sum()), worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("mu", [0.0, 3.0, 50.0])
def test_identity_equal_rating_sums(mu):
    """every user's rating sum is s: Dirichlet(mu) is Jelinek-Mercer with lambda = mu / (s + mu)"""
    u, i, s, total = equal_sum_data(40, 60)
    lam = mu / (total + mu)
    mc = (np.arange(40) % 3).astype(np.int32)
    cl = (np.arange(1, 41, dtype=np.int32), mc)
    ref = oracle.rm2(u, i, s, lam=lam, number_of_items=60, number_of_recommendations=1 << 30, number_of_clusters=3, map_user=cl[0], map_cluster=cl[1])
    assert_same_scores(definition_full(u, i, s, "dirichlet", mu, 60, clustering=cl), ref, ULP32)
    a = definition_full(u, i, s, "dirichlet", mu, 60, clustering=cl, score_dtype=np.float64)
    b = definition_full(u, i, s, "jm", lam, 60, clustering=cl, score_dtype=np.float64)
    print("Dirichlet mu = %g against JM lambda = %g: worst relative difference %.2e" % (mu, lam, assert_same_scores(a, b, 1e-12)))


@pytest.mark.parametrize("delta", [0.0, 0.5, 2.0])
def test_identity_equal_ratings(delta):
    """every rating is r0: absolute discounting(delta) is Jelinek-Mercer with lambda = delta / r0"""
    u, i, s, r0 = equal_rating_data(40, 60)
    lam = delta / r0
    mc = (np.arange(40) % 3).astype(np.int32)
    cl = (np.arange(1, 41, dtype=np.int32), mc)
    ref = oracle.rm2(u, i, s, lam=lam, number_of_items=60, number_of_recommendations=1 << 30, number_of_clusters=3, map_user=cl[0], map_cluster=cl[1])
    assert_same_scores(definition_full(u, i, s, "absoluteDiscounting", delta, 60, clustering=cl), ref, ULP32)
    a = definition_full(u, i, s, "absoluteDiscounting", delta, 60, clustering=cl, score_dtype=np.float64)
    b = definition_full(u, i, s, "jm", lam, 60, clustering=cl, score_dtype=np.float64)
    print("absolute discounting delta = %g against JM lambda = %g: worst relative difference %.2e" % (delta, lam, assert_same_scores(a, b, 1e-12)))


def base_conf():
    conf = pkg().Configuration()
    conf.setInt("numberOfItems", 10)
    conf.setInt("numberOfClusters", 2)
    return conf


def test_params_map_the_smoothing_keys():
    P = pkg()
    p = P.RM2Job(base_conf())._params(0, 1, 0)
    assert (p.flags, p.lambda_) == (0, 0.1)                        # the default: Jelinek-Mercer with the driver's lambda
    for name in ("jm", "JM"):
        conf = base_conf()
        conf.set("smoothing", name)
        conf.set("lambda", "0.25")
        conf.set("mu", "100")                                      # read for its own method only
        p = P.RM2Job(conf)._params(0, 1, 0)
        assert (p.flags, p.lambda_) == (0, 0.25)
    for name in ("dirichlet", "Dirichlet", "DIRICHLET"):
        conf = base_conf()
        conf.set("smoothing", name)
        conf.set("mu", "100")
        p = P.RM2Job(conf)._params(1, 3, 0)
        assert (p.flags, p.lambda_, p.rank, p.world) == (2, 100.0, 1, 3)
    for name in ("absoluteDiscounting", "absolutediscounting"):
        conf = base_conf()
        conf.set("smoothing", name)
        conf.set("delta", "0.5")
        conf.set("lambda", "0.9")
        p = P.RM2Job(conf)._params(0, 1, 0)
        assert (p.flags, p.lambda_) == (4, 0.5)
    assert "smoothing" not in P.Configuration.DEFAULTS and "mu" not in P.Configuration.DEFAULTS and "delta" not in P.Configuration.DEFAULTS


def test_params_refuse_an_unknown_name_and_a_missing_parameter():
    P = pkg()
    conf = base_conf()
    conf.set("smoothing", "laplace")
    with pytest.raises(ValueError, match="smoothing"):
        P.RM2Job(conf)._params(0, 1, 0)
    for name, other in (("dirichlet", "delta"), ("absoluteDiscounting", "mu")):
        conf = base_conf()
        conf.set("smoothing", name)
        conf.set(other, "1")                                       # the other method's parameter does not count
        with pytest.raises(ValueError, match="needs"):
            P.RM2Job(conf)._params(0, 1, 0)


def test_driver_hands_the_keys_to_the_rm2_stage():
    P = pkg()
    conf = P.Configuration()
    conf.set("smoothing", "dirichlet")
    conf.set("mu", "100")
    stage = P.RMRecommenderDriver(conf)._stage_conf(numberOfClusters=4)
    stage.setInt("numberOfItems", 10)
    p = P.RM2Job(stage)._params(0, 1, 0)
    assert (p.flags, p.lambda_, p.number_of_clusters) == (2, 100.0, 4)


def test_header_and_bindings_agree_on_the_flag_bits():
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "filmyou.h")) as f:
        h = f.read()
    bits = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+FY_RM2_(\w+)\s+(\d+)u", h)}
    assert bits == {"NO_CACHE": 1, "SMOOTHING_DIRICHLET": 2, "SMOOTHING_ABSOLUTE_DISCOUNT": 4}
    S = pkg().RM2Job.SMOOTHING
    assert (S["dirichlet"][0], S["absolutediscounting"][0], S["jm"][0]) == (2, 4, 0)


def test_null_context_is_refused_as_before():
    """without a device the parameters are never looked at: a NULL context answers FY_ERR_INVALID_ARGUMENT whatever the flags say"""
    native = __import__("importlib").import_module("filmyou-core_amd._native")
    lib = native.load()
    out = C.c_void_p()
    for flags, lam in ((0, 0.1), (2, 100.0), (4, 0.5), (6, 1.0), (2, -1.0)):
        p = native.RM2Params(lam, 10, 10, 0, 1, 0, 1, flags, 0)
        assert lib.fy_rm2_prepare(None, C.byref(p), None, 0, None, None, None, C.byref(out)) == -1
        assert b"NULL" in lib.fy_last_error()
