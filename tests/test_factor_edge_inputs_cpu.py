"""The inputs of the chunk, grid and k limit tests (factor_edge_inputs.py) against the constants of the kernels they are built
around, read from the sources: a changed chunk size, k limit or grid cap fails here instead of quietly turning those tests into
small-shape tests.  And the oracle alone on the long-row input in two entry orders: summation order moves it far less than the
tolerance the GPU tests use."""
import os
import re

import numpy as np
import pytest

import factor_edge_inputs as FE
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filmyou-core_amd", "csrc")


def _product(text):
    out = 1
    for f in text.split("*"):
        out *= int(f)
    return out


@pytest.fixture(scope="module")
def limits():
    def source(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()
    nmf, refine, cluster = source("fy_nmf.hip"), source("fy_refine.hip"), source("fy_cluster.hip")

    def const(src, name):
        m = re.search(r"constexpr int %s = (\d+);" % name, src)
        assert m, name
        return int(m.group(1))

    def grid(src, name):
        m = re.search(r"%s\(int64_t n, int block = (\d+), int cap = ([\d *]+)\)" % name, src)
        assert m, name
        return int(m.group(1)), _product(m.group(2))
    L = {"NMF_CHUNK": const(nmf, "NMF_CHUNK"), "NMF_MAX_K": const(nmf, "NMF_MAX_K"), "RF_CHUNK": const(refine, "RF_CHUNK"),
         "RF_MAX_K": const(refine, "RF_MAX_K"), "NMF_GRAM_BLOCKS": const(nmf, "NMF_GRAM_BLOCKS"), "grid_for": grid(source("fy_common.hpp"), "grid_for"), "rf_grid": grid(refine, "rf_grid")}
    m = re.search(r"grid_thread = .*?min<int64_t>\((\d+), \(\(int64_t\)n_rows \+ 255\) / 256\)", cluster)
    w = re.search(r"grid_wave = .*?min<int64_t>\((\d+), \(\(int64_t\)n_rows \+ 3\) / 4\)", cluster)
    assert m and w
    L["argmax_thread_rows"], L["argmax_wave_rows"] = int(m.group(1)) * 256, int(w.group(1)) * 4
    return L


def test_hubs_straddle_the_nmf_chunk(limits):
    d = FE.hubs()
    c = limits["NMF_CHUNK"]
    assert set(FE.HUB_USER_LENGTHS) == {c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 2 * c + 2, 2 * c + 3}
    # the four-way walk ends a chunk with 0, 1, 2 and 3 entries left over, in a first chunk and in a last one
    assert {(n % c) % 4 for n in FE.HUB_USER_LENGTHS if n > 2 * c} == {1, 2, 3} and (2 * c) % 4 == 0 and (c - 1) % 4 == 3 and c % 4 == 0
    assert all(n > c for n in FE.HUB_ITEM_LENGTHS) and max(FE.HUB_ITEM_LENGTHS) > 2 * c
    assert {n % c for n in FE.HUB_ITEM_LENGTHS} >= {1, 2, 3}
    assert d["user_lengths"][d["hub_users"] - 1].tolist() == list(FE.HUB_USER_LENGTHS)
    assert d["item_lengths"][d["hub_items"] - 1].tolist() == list(FE.HUB_ITEM_LENGTHS)
    # everybody else stays in one chunk: the hubs are the multi-chunk rows, and most chunks are single
    assert np.sort(d["user_lengths"])[-len(FE.HUB_USER_LENGTHS) - 1] < c and np.sort(d["item_lengths"])[-len(FE.HUB_ITEM_LENGTHS) - 1] < c


def test_k_edges_straddle_the_register_arrays(limits):
    kmax = limits["NMF_MAX_K"]
    assert kmax == limits["RF_MAX_K"] and kmax % 64 == 0
    # 65 is test_random_vs_oracle's
    want = {63, 64, kmax} | {64 * j for j in range(2, kmax // 64)} | {64 * j + 1 for j in range(2, kmax // 64)}
    assert set(FE.K_EDGES) == want and FE.K_BEYOND == kmax + 1
    # the small matrix of the k edge test: fewer item rows than Gram blocks and more user rows (two per block, empty blocks behind)
    blocks = limits["NMF_GRAM_BLOCKS"]
    n_users, n_items = FE.K_EDGE_SHAPE
    assert n_items < blocks < n_users <= 2 * blocks


def test_wrap_exceeds_every_grid_cap(limits):
    d = FE.wrap()
    user, item, score = d["coo"]
    for name in ("grid_for", "rf_grid"):
        block, cap = limits[name]
        threads, waves = cap * block, cap * (block // 64)
        assert len(user) > threads, name                     # the passes over the ratings
        assert d["n_users"] > waves, name                    # wave per row (or per chunk: every user row is one chunk)
        assert d["n_users"] * FE.WRAP_K > threads, name      # thread per element of H
    assert FE.WRAP_PER_USER <= min(limits["NMF_CHUNK"], limits["RF_CHUNK"])
    assert d["item_lengths"].min() > limits["NMF_CHUNK"] and d["item_lengths"].min() > limits["RF_CHUNK"]
    # the refinement's wrap: one row per wave needs L = 64, i.e. 32 < k <= 64
    k = -(-d["n_users"] // FE.WRAP_USERS_PER_SUB_CLUSTER)
    assert 32 < k <= 64


def test_tall_exceeds_the_thread_per_row_launches(limits):
    d = FE.tall()
    block, cap = limits["grid_for"]
    assert d["n_users"] > cap * block                        # k_nmf_rowptr, k_nmf_check_rows, k_nmf_chunk_counts, k_nmf_chunk_rows
    assert limits["NMF_MAX_K"] ** 2 <= cap * block           # k_nmf_gram_sum cannot wrap at any k the library serves
    assert FE.TALL_K <= limits["NMF_MAX_K"]


def test_parents_straddle_the_refinement_chunk(limits):
    d = FE.parents()
    c = limits["RF_CHUNK"]
    (ua, ia), (ub, ib), _ = d["lengths"]
    assert 64 < -(-FE.PARENT_USERS[0] // 8) <= limits["RF_MAX_K"] and -(-FE.PARENT_USERS[1] // 8) == 5 and -(-FE.PARENT_USERS[0] // 120) == 5
    assert set(FE.PARENT_A_ITEM_LENGTHS) == {FE.PARENT_USERS[0], c + 1, 2 * c + 3} and FE.PARENT_USERS[0] > 2 * c
    assert FE.PARENT_A_USER_LENGTHS[0] > 2 * c and FE.PARENT_A_USER_LENGTHS[0] % c % 4 == 0
    assert set(FE.PARENT_B_USER_LENGTHS) == {c - 1, c, c + 1, c + 2, 2 * c - 1, 2 * c + 1}
    assert {n % c % 4 for n in FE.PARENT_B_USER_LENGTHS + FE.PARENT_A_ITEM_LENGTHS} == {0, 1, 2, 3}
    assert ia.max() == FE.PARENT_USERS[0] and ua.max() == FE.PARENT_A_USER_LENGTHS[0] and ub.max() == max(FE.PARENT_B_USER_LENGTHS)


def test_assign_shapes_exceed_the_argmax_grids(limits):
    assert FE.ASSIGN_WIDE_ROWS > limits["argmax_wave_rows"] and FE.ASSIGN_THREAD_ROWS > limits["argmax_thread_rows"]


@pytest.mark.parametrize("k,ppc,norm,iters", [(3, True, -1, 4), (65, True, 2, 4)])
def test_oracle_alone_is_far_inside_the_tolerance(k, ppc, norm, iters):
    """The GPU sums a row in sorted order and by chunks, the oracle in input order: the oracle on a permuted COO shows what the
    order alone does -- asserted at 1e-12, two orders under the GPU tests' 1e-10."""
    d = FE.hubs()
    u, i, s = d["coo"]
    rng = np.random.default_rng(k)
    H0, W0 = rng.random((d["n_users"], k)) + 0.01, rng.random((d["n_items"], k)) + 0.01
    Ha, Wa = oracle.nmf(u, i, s, H0, W0, iterations=iters, ppc=ppc, normalization_frequency=norm)
    order = np.lexsort((i, u))[::-1]
    Hb, Wb = oracle.nmf(u[order], i[order], s[order], H0, W0, iterations=iters, ppc=ppc, normalization_frequency=norm)
    assert np.isfinite(Ha).all() and np.isfinite(Wa).all() and (Ha > 0).all()
    worst = max(np.max(np.abs(Ha - Hb) / np.abs(Ha)), np.max(np.abs(Wa - Wb) / np.maximum(np.abs(Wa), 1e-300)))
    print("k %d: worst relative difference between two entry orders %.3e" % (k, worst))
    np.testing.assert_allclose(Hb, Ha, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(Wb, Wa, rtol=1e-12, atol=1e-300)
