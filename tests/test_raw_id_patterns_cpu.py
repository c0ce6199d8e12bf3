"""tests/raw_id_patterns.py: every pattern is what its name says, sits on the gate it is named for, and the three CPU oracles are
invariant under it -- so the oracle of the dense job is a valid yardstick for a GPU job on ids up to 2^31 - 1."""
import functools

import numpy as np
import pytest

import oracle
import raw_id_patterns as rip

U, I, N_MAP, K = 40, 70, 37, 3
PATTERNS = rip.patterns(U, I, N_MAP)
INT32_MAX = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def dataset():
    """40 users x 70 items, about a third rated, half stars; a clustering map of 37 of the users over 3 clusters (the rest: cluster 0)."""
    rng = np.random.default_rng(20261020)
    rated = rng.random((U, I)) < 0.34
    rated[:, 0] = True                      # nobody without a rating
    rated[0, :] = True                      # every item rated
    user, item = np.nonzero(rated)
    score = (0.5 * rng.integers(1, 11, len(user))).astype(np.float32)
    map_user = np.sort(rng.choice(np.arange(1, U + 1), N_MAP, replace=False)).astype(np.int32)
    map_cluster = rng.integers(0, K, N_MAP).astype(np.int32)
    return (user + 1).astype(np.int32), (item + 1).astype(np.int32), score, map_user, map_cluster


def test_the_patterns_are_what_they_say():
    assert set(PATTERNS) >= {"dense", "zero_based", "netflix_like", "routing_edge_table", "routing_edge_sort", "pack_edge_64", "pack_edge_65",
                             "pack_edge_k_64", "pack_edge_k_65", "pow2_item_lo", "pow2_item_hi", "refine_edge_on", "refine_edge_off",
                             "int32_edge", "int32_user_packed", "shard_edge_on", "shard_edge_off"}
    for name, (f, g) in PATTERNS.items():
        assert f.dtype == g.dtype == np.int64 and len(f) == U and len(g) == I, name
        assert np.all(np.diff(f) > 0) and np.all(np.diff(g) > 0), name
        assert f[0] >= 0 and g[0] >= 0 and f[-1] <= INT32_MAX and g[-1] <= INT32_MAX, name
        assert np.array_equal(f.astype(np.int32), f) and np.array_equal(g.astype(np.int32), g), name
    ends = lambda name: tuple(int(x) for x in (PATTERNS[name][0][0], PATTERNS[name][0][-1], PATTERNS[name][1][0], PATTERNS[name][1][-1]))
    assert ends("dense") == (1, U, 1, I)
    assert ends("zero_based") == (0, U - 1, 0, I - 1)
    assert ends("netflix_like")[1::2] == (2649429, 209171)
    assert ends("pack_edge_64")[1::2] == (2 ** 24 - 2, 2 ** 24 - 1) and ends("pack_edge_65")[1::2] == (2 ** 24 - 1, 2 ** 24 - 1)
    assert ends("pack_edge_k_64")[1::2] == (2 ** 23 - 2, 2 ** 24 - 1) and ends("pack_edge_k_65")[1::2] == (2 ** 23 - 1, 2 ** 24 - 1)
    assert ends("pow2_item_lo")[3] == 2 ** 16 - 1 and ends("pow2_item_hi")[3] == 2 ** 16
    assert ends("refine_edge_on")[3] == 2 ** 28 - 1 and ends("refine_edge_off")[3] == 2 ** 28
    assert ends("int32_edge") == (0, INT32_MAX, 0, INT32_MAX)
    # ids above 2^30 that are not the maximum: a sign or a shift lost in the middle of the range shows too
    assert np.sum(PATTERNS["int32_edge"][0] > 2 ** 30) > 2 and np.sum(PATTERNS["int32_edge"][1] > 2 ** 30) > 2


def test_every_pattern_sits_on_its_gate():
    """The gates in Python, with the constants as they stand in the source (tests/raw_id_patterns.py names file and expression of each)."""
    mx = lambda name: (int(PATTERNS[name][0][-1]), int(PATTERNS[name][1][-1]))
    # fy_prep.hip, build_structure: `n_map > 0 && nRU <= 8 * n_map + (1 << 20)`
    assert mx("routing_edge_table")[0] + 1 == 8 * N_MAP + (1 << 20) and rip.routing_by_table(mx("routing_edge_table")[0], N_MAP)
    assert mx("routing_edge_sort")[0] + 1 == 8 * N_MAP + (1 << 20) + 1 and not rip.routing_by_table(mx("routing_edge_sort")[0], N_MAP)
    assert rip.routing_by_table(mx("dense")[0], N_MAP)
    assert not rip.routing_by_table(mx("netflix_like")[0], N_MAP) and not rip.routing_by_table(mx("netflix_like")[0], 190000)
    assert not rip.routing_by_table(mx("int32_edge")[0], N_MAP)
    # fy_prep.hip, build_structure: `ib0 + ub0 + 16 <= 64 && kb0 + ib0 + ub0 + 16 <= 64`
    assert rip.key_bits(*mx("pack_edge_64"), 1) == (24, 24, 0) and rip.packed_gate(*mx("pack_edge_64"), 1)
    assert rip.key_bits(*mx("pack_edge_65"), 1) == (24, 25, 0) and not rip.packed_gate(*mx("pack_edge_65"), 1)
    assert rip.key_bits(*mx("pack_edge_k_64"), 2) == (24, 23, 1) and rip.packed_gate(*mx("pack_edge_k_64"), 2)
    assert rip.key_bits(*mx("pack_edge_k_65"), 2) == (24, 24, 1) and not rip.packed_gate(*mx("pack_edge_k_65"), 2)
    assert rip.packed_gate(*mx("pack_edge_k_65"), 1), "only the cluster bits close the gate for pack_edge_k_65"
    assert rip.key_bits(*mx("int32_edge"), 1) == (31, 32, 0) and not rip.packed_gate(*mx("int32_edge"), 1)
    assert rip.key_bits(*mx("int32_user_packed"), 1) == (16, 32, 0) and rip.packed_gate(*mx("int32_user_packed"), 1)
    assert rip.packed_gate(*mx("dense"), 3) and rip.packed_gate(*mx("netflix_like"), 3)
    # fy_prep.hip, build_structure: `ib = bits_for(max_item)`
    assert rip.key_bits(*mx("pow2_item_lo"), 1)[0] == 16 and rip.key_bits(*mx("pow2_item_hi"), 1)[0] == 17
    # fy_rm2.hip, C.refine: `max_item < (1 << 28)`
    assert rip.refinement_allowed(mx("refine_edge_on")[1]) and rip.refinement_allowed(mx("dense")[1])
    assert not rip.refinement_allowed(mx("refine_edge_off")[1]) and not rip.refinement_allowed(mx("int32_edge")[1])
    # fy_prep.hip, shard_ratings_by_cluster: `nRU + nRI > 2^25`
    on, off = mx("shard_edge_on"), mx("shard_edge_off")
    assert on[0] + 1 + on[1] + 1 == 1 << 25 and rip.sharded_prep_allowed(*on)
    assert off[0] + 1 + off[1] + 1 == (1 << 25) + 1 and not rip.sharded_prep_allowed(*off)


def test_relabel_and_back():
    f, g = PATTERNS["int32_edge"]
    user, item, score, _, _ = dataset()
    ru, ri, rs = rip.relabel_triples((user, item, score), f, g)
    assert ru.dtype == ri.dtype == np.int32 and ru.min() == 0 and ru.max() == INT32_MAX and ri.min() == 0 and ri.max() == INT32_MAX
    assert np.array_equal(rip.unlabel(ru, f), user) and np.array_equal(rip.unlabel(ri, g), item)
    assert np.array_equal(rip.relabel(np.array([-5, 1, U]), f), [-5, 0, INT32_MAX])
    with pytest.raises(AssertionError):
        rip.unlabel(np.array([1]), f)          # the ramp goes 0, 1 + 2^31 / 39^2, ...: 1 is none of its ids
    back = rip.map_back({"user": ru, "item": ri, "score": rs, "total_sum": 1.5}, f, g)
    assert np.array_equal(back["user"], user) and np.array_equal(back["item"], item) and back["score"] is rs and back["total_sum"] == 1.5


def same_bytes(a, b, keys):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert x.tobytes() == y.tobytes(), k


@functools.lru_cache(maxsize=None)
def dense_oracles():
    user, item, score, mu, mc = dataset()
    rm2 = oracle.rm2(user, item, score, lam=0.3, number_of_items=I, number_of_recommendations=1 << 30, number_of_clusters=K,
                     map_user=mu, map_cluster=mc)
    sim = oracle.itemsim(user, item, score, max_similarities_per_item=12)
    cf = oracle.itemcf(user, item, score, sim["item"], sim["other"], sim["sim"], num_recommendations=9, max_prefs_per_user=15)
    return rm2, sim, cf


RM2_KEYS = ("rec_user", "rec_item", "rec_cluster", "rec_score", "user_id", "user_sum", "item_id", "item_coll", "item_sum", "total_sum")


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_the_oracles_are_invariant(name):
    f, g = PATTERNS[name]
    user, item, score, mu, mc = dataset()
    ru, ri, rs = rip.relabel_triples((user, item, score), f, g)
    rm2_0, sim_0, cf_0 = dense_oracles()
    assert len(rm2_0["rec_user"]) > 1000 and len(sim_0["item"]) > 500 and len(cf_0["user"]) > 300
    rm2 = oracle.rm2(ru, ri, rs, lam=0.3, number_of_items=I, number_of_recommendations=1 << 30, number_of_clusters=K,
                     map_user=rip.relabel(mu, f), map_cluster=mc)
    same_bytes(rip.map_back(rm2, f, g), rm2_0, RM2_KEYS)
    sim = oracle.itemsim(ru, ri, rs, max_similarities_per_item=12)
    same_bytes(rip.map_back(sim, f, g), sim_0, ("item", "other", "sim", "pairs"))
    cf = oracle.itemcf(ru, ri, rs, sim["item"], sim["other"], sim["sim"], num_recommendations=9, max_prefs_per_user=15)
    same_bytes(rip.map_back(cf, f, g), cf_0, ("user", "item", "score"))
