"""NMF / PPC factorisation (fy_nmf_factorize) against the reference's own vectors (NMFTestData / PPCTestData: one and ten
iterations from W_init / H_init, asserted by the reference with accuracy 1e-4) and against the oracle on random sparse data,
including the L1-normalisation branch the reference's vectors never reach; then the whole chain factorise -> assign.  The inputs
of factor_edge_inputs.py take the same comparison to rows of several chunks, launches whose grid-stride loops wrap (by wave and element at 17 000 rows, by row above 1 048 576), every k at
which the register arrays or the k x k matrix change, and initial matrices that overflow into the infinity clamps."""
import functools
import json
import os

import numpy as np
import pytest

import factor_edge_inputs as FE
import oracle
from util import pkg

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factorization_test_data.json")


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def coo(A):
    A = np.array(A)
    i, u = np.nonzero(A > 0)
    return (u + 1).astype(np.int32), (i + 1).astype(np.int32), A[i, u].astype(np.float32)


def conf_for(P, n_users, n_items, k, iterations, norm=None):
    conf = P.Configuration()
    conf.setInt("numberOfUsers", n_users)
    conf.setInt("numberOfItems", n_items)
    conf.setInt("numberOfClusters", k)
    conf.setInt("numberOfIterations", iterations)
    if norm is not None:
        conf.setInt("normalizationFrequency", norm)
    return conf


@pytest.mark.parametrize("name,ppc", [("nmf", False), ("ppc", True)])
@pytest.mark.parametrize("iterations,suffix", [(1, "one"), (10, "ten")])
def test_reference_vectors(ctx, golden, name, ppc, iterations, suffix):
    P = pkg()
    d = golden[name]
    H, W = P.NMFDriver(conf_for(P, 30, 100, 10, iterations, norm=12), ctx, ppc=ppc).run(coo(d["A"]), d["H_init"], d["W_init"])
    # the reference asserts 1e-4 (HadoopIntegrationTest.accuracy); fp64 on both sides agrees far better
    np.testing.assert_allclose(H, np.array(d["H_" + suffix]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(W, np.array(d["W_" + suffix]), rtol=0, atol=1e-9)


def test_ppc_toy(ctx, golden):
    P = pkg()
    d = golden["ppc"]
    H, _ = P.NMFDriver(conf_for(P, 7, 5, 2, 1, norm=12), ctx, ppc=True).run(coo(d["Ap"]), d["h0p"], d["w0p"])
    np.testing.assert_allclose(H, np.array(d["h1p"]), rtol=0, atol=1e-7)     # Ap goes through FloatWritable: 3 decimals as fp32


@pytest.mark.parametrize("n_users,n_items,k,ppc,norm,iters", [(300, 200, 7, False, 0, 3), (500, 120, 50, True, -1, 4),
                                                              (257, 333, 65, True, 2, 4), (64, 64, 200, False, 0, 2)])
def test_random_vs_oracle(ctx, n_users, n_items, k, ppc, norm, iters):
    P = pkg()
    rng = np.random.default_rng(n_users + 7 * k)
    A = (rng.random((n_items, n_users)) < 0.15) * rng.integers(1, 6, (n_items, n_users))
    A[rng.integers(0, n_items, n_users), np.arange(n_users)] = 3          # every user rates something
    A[np.arange(n_items), rng.integers(0, n_users, n_items)] = 4          # every item is rated
    u, i, s = coo(A)
    s = np.r_[s, [0.0, -1.0]].astype(np.float32)                            # dropped by score > 0
    u, i = np.r_[u, [1, 2]].astype(np.int32), np.r_[i, [1, 1]].astype(np.int32)
    s = np.r_[s, [2.5]].astype(np.float32)                                  # one pair twice (the scores above are whole numbers): both count
    u, i = np.r_[u, u[:1]].astype(np.int32), np.r_[i, i[:1]].astype(np.int32)
    assert s[0] > 0 and s[0] != s[-1]
    H0, W0 = rng.random((n_users, k)) + 0.01, rng.random((n_items, k)) + 0.01
    H, W = P.NMFDriver(conf_for(P, n_users, n_items, k, iters, norm=norm), ctx, ppc=ppc).run((u, i, s), H0, W0)
    Ho, Wo = oracle.nmf(u, i, s, H0, W0, iterations=iters, ppc=ppc, normalization_frequency=norm)
    np.testing.assert_allclose(H, Ho, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(W, Wo, rtol=1e-10, atol=1e-300)
    if ppc and norm == -1:
        np.testing.assert_allclose(np.abs(H).sum(1), 1.0, rtol=1e-12)       # normalised every iteration


@pytest.mark.parametrize("k,ppc,norm,iters", [(3, True, -1, 4), (64, False, 0, 3), (65, True, 2, 4), (256, False, 0, 2)])
def test_long_rows_vs_oracle(ctx, k, ppc, norm, iters):
    """Rows of one chunk less one entry up to three chunks (FE.hubs): the chunk table, the partials' sum in chunk order and the
    four-way walk's tail at a chunk end, on both sides of the matrix."""
    P = pkg()
    d = FE.hubs()
    u, i, s = d["coo"]
    rng = np.random.default_rng(1000 + k)
    H0, W0 = rng.random((d["n_users"], k)) + 0.01, rng.random((d["n_items"], k)) + 0.01
    H, W = P.NMFDriver(conf_for(P, d["n_users"], d["n_items"], k, iters, norm=norm), ctx, ppc=ppc).run((u, i, s), H0, W0)
    Ho, Wo = oracle.nmf(u, i, s, H0, W0, iterations=iters, ppc=ppc, normalization_frequency=norm)
    hub_u, hub_i = d["hub_users"] - 1, d["hub_items"] - 1
    print("k %d: worst relative error H %.3e W %.3e; hub users %s; hub items %s" % (
        k, FE.worst_relative(H, Ho), FE.worst_relative(W, Wo), ["%.1e" % FE.worst_relative(H[r], Ho[r]) for r in hub_u],
        ["%.1e" % FE.worst_relative(W[r], Wo[r]) for r in hub_i]))
    np.testing.assert_allclose(H, Ho, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(W, Wo, rtol=1e-10, atol=1e-300)
    if ppc and norm == -1:
        np.testing.assert_allclose(np.abs(H).sum(1), 1.0, rtol=1e-12)


@pytest.mark.parametrize("ppc,norm", [(True, 2), (False, 0)])
def test_grid_stride_wraps_vs_oracle(ctx, ppc, norm):
    """FE.wrap: more ratings, chunks, rows and elements of H than one launch has threads or waves, so the loops of k_nmf_keys,
    k_nmf_spmm_chunks, k_nmf_update and k_nmf_spmm_reduce go round more than once (test_tall_matrix_vs_oracle has the rest)."""
    P = pkg()
    d = FE.wrap()
    u, i, s = d["coo"]
    k, iters = FE.WRAP_K, 2
    rng = np.random.default_rng(17)
    H0, W0 = rng.random((d["n_users"], k)) + 0.01, rng.random((d["n_items"], k)) + 0.01
    H, W = P.NMFDriver(conf_for(P, d["n_users"], d["n_items"], k, iters, norm=norm), ctx, ppc=ppc).run((u, i, s), H0, W0)
    Ho, Wo = oracle.nmf(u, i, s, H0, W0, iterations=iters, ppc=ppc, normalization_frequency=norm)
    print("wrap ppc %d: worst relative error H %.3e W %.3e" % (ppc, FE.worst_relative(H, Ho), FE.worst_relative(W, Wo)))
    # a row the wrapped loop passed over keeps what the buffer held
    assert not (H == H0).all(1).any() and not (W == W0).all(1).any()
    assert not (Ho == H0).all(1).any() and not (Wo == W0).all(1).any()
    np.testing.assert_allclose(H, Ho, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(W, Wo, rtol=1e-10, atol=1e-300)


@pytest.mark.parametrize("ppc,norm", [(True, 1), (False, 0)])
def test_tall_matrix_vs_oracle(ctx, ppc, norm):
    """FE.tall: more user rows than one launch has threads, so the thread-per-row loops that build the row pointers, the
    empty-row check and the chunk tables go round more than once; a row they passed over would be walked from a stale table.
    Sums over a million rows move with their order: the oracle alone differs by 2.7e-14 between two entry orders here."""
    P = pkg()
    d = FE.tall()
    u, i, s = d["coo"]
    k, iters = FE.TALL_K, 2
    rng = np.random.default_rng(23)
    H0, W0 = rng.random((d["n_users"], k)) + 0.01, rng.random((d["n_items"], k)) + 0.01
    H, W = P.NMFDriver(conf_for(P, d["n_users"], d["n_items"], k, iters, norm=norm), ctx, ppc=ppc).run((u, i, s), H0, W0)
    Ho, Wo = oracle.nmf(u, i, s, H0, W0, iterations=iters, ppc=ppc, normalization_frequency=norm)
    print("tall ppc %d: worst relative error H %.3e W %.3e" % (ppc, FE.worst_relative(H, Ho), FE.worst_relative(W, Wo)))
    assert not (H == H0).all(1).any() and not (W == W0).all(1).any()
    np.testing.assert_allclose(H, Ho, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(W, Wo, rtol=1e-10, atol=1e-300)
    if ppc:
        np.testing.assert_allclose(np.abs(H).sum(1), 1.0, rtol=1e-12)       # normalised every iteration


@functools.lru_cache(maxsize=None)
def k_edge_input():
    n_users, n_items = FE.K_EDGE_SHAPE
    rng = np.random.default_rng(257130)
    A = (rng.random((n_items, n_users)) < 0.15) * rng.integers(1, 6, (n_items, n_users))
    A[rng.integers(0, n_items, n_users), np.arange(n_users)] = 3          # every user rates something
    A[np.arange(n_items), rng.integers(0, n_users, n_items)] = 4          # every item is rated
    return coo(A)


@pytest.mark.parametrize("k", FE.K_EDGES)
def test_k_edges_vs_oracle(ctx, k):
    """Every k at which a lane gains a column of the register arrays, the last k with the k x k matrix in LDS, and the limit."""
    P = pkg()
    n_users, n_items = FE.K_EDGE_SHAPE
    u, i, s = k_edge_input()
    rng = np.random.default_rng(k)
    H0, W0 = rng.random((n_users, k)) + 0.01, rng.random((n_items, k)) + 0.01
    H, W = P.NMFDriver(conf_for(P, n_users, n_items, k, 2, norm=2), ctx, ppc=True).run((u, i, s), H0, W0)
    Ho, Wo = oracle.nmf(u, i, s, H0, W0, iterations=2, ppc=True, normalization_frequency=2)
    print("k %d: worst relative error H %.3e W %.3e" % (k, FE.worst_relative(H, Ho), FE.worst_relative(W, Wo)))
    np.testing.assert_allclose(H, Ho, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(W, Wo, rtol=1e-10, atol=1e-300)


def test_k_beyond_the_limit_is_refused(ctx):
    P = pkg()
    n_users, n_items = FE.K_EDGE_SHAPE
    k = FE.K_BEYOND
    with pytest.raises(RuntimeError, match="exceeds the kernel limit 256"):
        P.NMFDriver(conf_for(P, n_users, n_items, k, 1), ctx, ppc=True).run(k_edge_input(), np.ones((n_users, k)), np.ones((n_items, k)))


@pytest.mark.parametrize("ppc,norm", [(True, 0), (True, -1), (False, 0)])
@pytest.mark.parametrize("iters", [1, 2])
def test_infinities_are_clamped_like_the_reference(ctx, ppc, norm, iters):
    """Initial matrices around 1e200 make W^T W, C h and the PPC sums infinite: the reference replaces an infinite X + d, Y + e
    (PPC) or X, Y (the W update) by Double.MAX_VALUE and goes on with finite numbers.  Plain NMF leaves exact zeros in H."""
    P = pkg()
    n_users, n_items, k = 70, 40, 5
    rng = np.random.default_rng(7040)
    A = (rng.random((n_items, n_users)) < 0.2) * rng.integers(1, 6, (n_items, n_users))
    A[rng.integers(0, n_items, n_users), np.arange(n_users)] = 3
    A[np.arange(n_items), rng.integers(0, n_users, n_items)] = 4
    u, i, s = coo(A)
    H0, W0 = FE.huge_initial(rng, (n_users, k)), FE.huge_initial(rng, (n_items, k))
    Ho, Wo = oracle.nmf(u, i, s, H0, W0, iterations=iters, ppc=ppc, normalization_frequency=norm)
    assert np.isfinite(Ho).all() and np.isfinite(Wo).all()                  # otherwise the comparison would be NaN = NaN
    assert (Ho > 0).all() if ppc else (Ho == 0).all()
    assert (Wo > 0).all() if ppc or iters == 1 else (Wo == 0).all()         # plain NMF: W follows H to zero one iteration later
    if ppc:                                                                 # the case does need the clamp: without it, inf / inf
        assert np.isnan(FE.unclamped_ppc_row(u, i, s, H0, W0, 0)).all()
    with np.errstate(over="ignore"):
        assert np.isinf(W0.T @ W0).all() and np.isinf(H0.T @ H0).all()      # both k x k matrices overflow: the W update clamps Y
    H, W = P.NMFDriver(conf_for(P, n_users, n_items, k, iters, norm=norm), ctx, ppc=ppc).run((u, i, s), H0, W0)
    assert np.isfinite(H).all() and np.isfinite(W).all()
    print("clamp ppc %d norm %d iterations %d: worst relative error H %.3e W %.3e" % (ppc, norm, iters, FE.worst_relative(H, Ho), FE.worst_relative(W, Wo)))
    np.testing.assert_allclose(H, Ho, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(W, Wo, rtol=1e-10, atol=1e-300)


def test_errors_mirror_the_reference(ctx):
    P = pkg()
    u, i, s = np.array([1, 2], np.int32), np.array([1, 1], np.int32), np.array([3, 4], np.float32)
    with pytest.raises(RuntimeError, match="User 3 has not rated any item"):
        P.NMFDriver(conf_for(P, 3, 1, 2, 1), ctx).run((u, i, s), np.ones((3, 2)), np.ones((1, 2)))
    with pytest.raises(RuntimeError, match="Item 2 has not been rated by anybody"):
        P.NMFDriver(conf_for(P, 2, 2, 2, 1), ctx).run((u, i, s), np.ones((2, 2)), np.ones((2, 2)))
    with pytest.raises(RuntimeError, match="outside"):
        P.NMFDriver(conf_for(P, 1, 1, 2, 1), ctx).run((u, i, s), np.ones((1, 2)), np.ones((1, 2)))


def test_chain_factorise_then_assign(ctx, golden):
    """PPC ten iterations -> cluster assignment: the argmax of the reference's H_ten, row by row"""
    P = pkg()
    d = golden["ppc"]
    H, _ = P.NMFDriver(conf_for(P, 30, 100, 10, 10, norm=12), ctx, ppc=True).run(coo(d["A"]), d["H_init"], d["W_init"])
    users, clusters, counts = P.ClusterAssignmentJob(ctx).run(H, first_user=1)
    assert clusters.tolist() == np.array(d["H_ten"]).argmax(1).tolist()
    assert counts.sum() == 30
