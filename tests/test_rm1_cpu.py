"""The RM1 estimator beside RM2: its plain statement (tests/rm1_definition.py) in its dense and its sparse form, pinned to a
brute-force product in extended precision and to a hand example; the host's `relevanceModel` key.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

from rm1_definition import definition_full, definition_sparse
from rm2_smoothing_definition import user_model
from util import pkg, synth

HAND = (np.array([1, 1, 2, 2, 2, 3, 3, 3, 4, 5, 5], dtype=np.int32), np.array([1, 2, 1, 2, 3, 1, 2, 4, 5, 1, 5], dtype=np.int32),
        np.array([4, 2, 5, 3, 1, 2, 2, 4, 3, 1, 5], dtype=np.float32))
HAND_FINITE_AT_0 = {(1, 3): -5.493061, (1, 4): -5.075174, (4, 1): -3.583519}      # every other candidate row is -inf at lambda = 0
HAND_AT_HALF = {(1, 5): -4.526865, (4, 1): -2.783762}                              # all 14 rows are finite at lambda = 0.5


def by_pair(ref):
    return {(int(a), int(b)): (float(c), int(d)) for a, b, c, d in zip(ref["rec_user"], ref["rec_item"], ref["rec_score"], ref["rec_cluster"])}


def assert_same_scores(got, want, rel):
    g, w = by_pair(got), by_pair(want)
    assert g.keys() == w.keys() and len(w) > 0
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


@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("method,param", [("jm", 0.1), ("jm", 0.5), ("dirichlet", 50.0), ("absoluteDiscounting", 0.5)])
def test_dense_equals_sparse_on_the_tiny_shape(method, param, K):
    S = synth()
    u, i, s, _ = S.generate("tiny")
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    uu = np.unique(u)
    cl = (uu, S.hash_clustering(uu, K))
    a = definition_full(u, i, s, method, param, clustering=cl, score_dtype=np.float64)
    b = definition_sparse(u, i, s, method, param, clustering=cl, score_dtype=np.float64)
    assert np.array_equal(a["rec_user"], b["rec_user"])
    worst = assert_same_scores(b, a, 1e-12)
    print("%s %g, %d clusters: %d rows, dense against sparse %.2e" % (method, param, K, len(a["rec_user"]), worst))
    assert a["rec_score"].max() < -40.0 and a["rec_score"].min() > -1300.0      # the purely relative criterion is well posed here


def brute_force(u, i, s, method, param, clustering):
    """score(u, i) by the triple loop: per neighbour the product c_vi prod_j c_vj as math.fsum of logs, then an exactly summed
    log-sum-exp over the neighbours"""
    keep = s > 0
    u, i, s = u[keep].astype(int), i[keep].astype(int), s[keep].astype(np.float64)
    su, nu, isum = {}, {}, {}
    for a, b, r in zip(u, i, s):
        su[a] = su.get(a, 0.0) + r
        nu[a] = nu.get(a, 0) + 1
        isum[b] = isum.get(b, 0.0) + r
    total = sum(math.floor(v) for v in su.values())
    cl_of = {int(a): int(b) for a, b in zip(*clustering)}
    x, beta_r, w = user_model(method, param, s, np.array([su[a] for a in u]), np.array([float(nu[a]) for a in u]))
    a_of = {(a, b): w * xv for a, b, xv in zip(u, i, x)}
    beta = {a: bv for a, bv in zip(u, beta_r)}
    out = {}
    for c in sorted({cl_of.get(a, 0) for a in su}):
        mem = sorted(a for a in su if cl_of.get(a, 0) == c)
        items = sorted({b for a, b in a_of if cl_of.get(a, 0) == c})
        cval = lambda v, j: a_of.get((v, j), 0.0) + beta[v] * isum[j] / total
        for uu in mem:
            J = [j for j in items if (uu, j) in a_of]
            for cand in items:
                if (uu, cand) in a_of:
                    continue
                logs = []
                for v in mem:
                    if v == uu:
                        continue
                    f = [cval(v, j) for j in J] + [cval(v, cand)]
                    if min(f) > 0.0:
                        logs.append(math.fsum(math.log(t) for t in f))
                if logs:
                    m = max(logs)
                    out[(uu, cand)] = (-math.log(len(mem)) + m + math.log(math.fsum(math.exp(t - m) for t in logs)), c)
                else:
                    out[(uu, cand)] = (-math.inf, c)
    return out


@pytest.mark.parametrize("method,param", [("jm", 0.5), ("jm", 0.0), ("dirichlet", 50.0), ("absoluteDiscounting", 1.0)])
def test_dense_statement_is_the_brute_force_product_on_the_reference_fixture(rm_golden, method, param):
    g = rm_golden
    u, i, s = g["coo"]
    cl = (g["map_user"], g["map_cluster"])
    assert len(set(g["map_cluster"].tolist())) == 5
    want = brute_force(u, i, s, method, param, cl)
    got = by_pair(definition_full(u, i, s, method, param, clustering=cl, score_dtype=np.float64))
    assert got.keys() == want.keys() and len(want) > 0
    worst = 0.0
    for k, (sw, cw) in want.items():
        sg, cg = got[k]
        assert cg == cw
        if math.isfinite(sw):
            worst = max(worst, abs(sg - sw) / abs(sw))
        else:
            assert sg == sw
    print("%s %g: %d rows, %d finite, worst relative difference %.2e" % (method, param, len(want), sum(math.isfinite(v[0]) for v in want.values()), worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("definition", [definition_full, definition_sparse])
def test_hand_example(definition):
    for method in ("jm", "dirichlet", "absoluteDiscounting"):       # lambda = 0, mu = 0 and delta = 0 are one model
        rows = by_pair(definition(*HAND, method, 0.0, score_dtype=np.float64))
        assert len(rows) == 14
        for k, (sc, c) in rows.items():
            assert c == 0
            if k in HAND_FINITE_AT_0:
                assert abs(sc - HAND_FINITE_AT_0[k]) <= 5e-7, (method, k, sc)
            else:
                assert sc == -math.inf, (method, k, sc)
    rows = by_pair(definition(*HAND, "jm", 0.5, score_dtype=np.float64))
    assert len(rows) == 14 and all(math.isfinite(v[0]) for v in rows.values())
    for k, want in HAND_AT_HALF.items():
        assert abs(rows[k][0] - want) <= 5e-7, (k, rows[k])


def base_conf():
    conf = pkg().Configuration()
    conf.setInt("numberOfItems", 10)
    conf.setInt("numberOfClusters", 1)
    conf.set("lambda", "0.1")
    return conf


def test_relevance_model_key():
    P = pkg()
    assert P.RM2Job(base_conf())._params(0, 1, 0).flags == 0                    # the default is rm2
    for name, bit in (("rm2", 0), ("RM2", 0), ("rm1", 8), ("RM1", 8), ("Rm1", 8)):
        conf = base_conf()
        conf.set("relevanceModel", name)
        assert P.RM2Job(conf)._params(0, 1, 0).flags == bit
    conf = base_conf()
    conf.set("relevanceModel", "rm1")
    conf.set("smoothing", "dirichlet")
    conf.set("mu", "100")
    p = P.RM2Job(conf)._params(1, 3, 0)
    assert (p.flags, p.lambda_, p.rank, p.world) == (10, 100.0, 1, 3)
    conf.set("smoothing", "absoluteDiscounting")
    conf.set("delta", "0.5")
    assert P.RM2Job(conf)._params(0, 1, 0).flags == 12
    for bad in ("rm3", "", "rm1 ", "relevance"):
        conf = base_conf()
        conf.set("relevanceModel", bad)
        with pytest.raises(ValueError, match="relevanceModel"):
            P.RM2Job(conf)._params(0, 1, 0)
    assert "relevanceModel" not in P.Configuration.DEFAULTS


def test_driver_hands_the_key_to_the_rm2_stage():
    P = pkg()
    conf = P.Configuration()
    conf.set("relevanceModel", "rm1")
    stage = P.RMRecommenderDriver(conf)._stage_conf(numberOfClusters=4)
    stage.setInt("numberOfItems", 10)
    stage.set("lambda", "0.1")
    p = P.RM2Job(stage)._params(0, 1, 0)
    assert (p.flags, p.number_of_clusters) == (8, 4)


def test_header_bindings_and_mirrors_agree_on_the_flag():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "filmyou.h")) as f:
        h = f.read()
    m = re.search(r"#define\s+FY_RM2_ESTIMATOR_RM1\s+(\w+)u\b", h)
    assert m and int(m.group(1), 0) == 8 == pkg().RM2Job.RELEVANCE_MODEL["rm1"]
    assert re.search(r"#define\s+FY_ABI_VERSION\s+5\b", h)
    with open(os.path.join(root, "filmyou-core_amd", "host", "filmyou_job.hpp")) as f:
        assert 'conf.get("relevanceModel", "rm2")' in f.read()
    with open(os.path.join(root, "filmyou-core_amd", "jni", "NativeRM2Job.java")) as f:
        assert "ESTIMATOR_RM1 = 8" in f.read()


def test_abi_version_stays_5():
    native = __import__("importlib").import_module("filmyou-core_amd._native")
    assert native.load().fy_abi_version() == 5
