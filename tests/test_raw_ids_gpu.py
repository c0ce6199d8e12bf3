"""Raw user and item ids that are sparse, large or 2^31 - 1, through every job (tests/raw_id_patterns.py).

The library depends on the raw ids through their order alone, so a job on relabelled ids, mapped back, must equal the job on dense ids
BYTE FOR BYTE -- rows, side outputs and every counter of the statistics -- and the dense job is checked against its oracle or definition
in the same test, so equality is never "equally wrong".  What differs between two patterns is the code chosen by the MAGNITUDE of the
ids: the field widths of the sort keys and the gate of the packed mode (fy_prep.hip, build_structure), the route of the clustering map
(host table / device sort + k_lookup_cluster), the refinement pass's raw-id table (fy_rm2.hip, C.refine), the sharded prep's gate.
tests/test_raw_id_patterns_cpu.py states every gate's inequality for the patterns used here; where the library reports the side taken
(rows_refined, stats_layout, blocks_total, panel_clusters) it is asserted here as well.  No tolerance of its own: oracle comparisons use
util.RTOL (RM2), test_itemcf_gpu.RTOL and the rules of itemsim_measures_ref.
"""
import functools
import os

import numpy as np
import pytest

import itemsim_measures_ref as MR
import oracle
import raw_id_patterns as rip
import refine_ref as RR
import test_cooc_epilogue_gpu as EPI
import test_itemcf_gpu as ICF
from test_score_walk_gpu import N_ITEMS as WALK_ITEMS, N_USERS as WALK_USERS, dataset as walk_dataset, reference as walk_reference
from util import RTOL, assert_topn_matches, pkg

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
FY_ERR_DUPLICATE_RATING, FY_ERR_NEGATIVE_ID, FY_ERR_UNSUPPORTED = -7, -8, -10


def copy_of(d):
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def counters(stats):
    """every field of the statistics that is no time"""
    return {k: v for k, v in stats.items() if not k.startswith("ms_")}


def assert_same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert x.tobytes() == y.tobytes(), k


class environment:
    """FY_* for the jobs of one context (the library reads them when the context is created)"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def half_star_data(n_users, n_items, density, seed):
    """dense 1-based ids, everybody rates something and everything is rated, half stars, shuffled COO"""
    rng = np.random.default_rng(seed)
    rated = rng.random((n_users, n_items)) < density
    rated[np.arange(n_users), rng.integers(0, n_items, n_users)] = True
    rated[rng.integers(0, n_users, n_items), np.arange(n_items)] = True
    user, item = np.nonzero(rated)
    order = rng.permutation(len(user))
    user, item = user[order], item[order]
    score = (0.5 * rng.integers(1, 11, len(user))).astype(np.float32)
    return (user + 1).astype(np.int32), (item + 1).astype(np.int32), score


# ------------------------------------------------------------------------------------------------ RM2, a small flat job
FLAT_U, FLAT_I, FLAT_LAM, FLAT_TOP = 48, 96, 0.3, 12
FLAT_UNMAPPED = (5, 19, 48)          # users the map does not name: cluster 0
FLAT_TWICE = 7                       # named twice, with different clusters: the later pair wins
FLAT_N_MAP = FLAT_U - len(FLAT_UNMAPPED) + 1 + 2


@functools.lru_cache(maxsize=None)
def flat_data():
    return half_star_data(FLAT_U, FLAT_I, 0.3, 20261021)


def flat_map(K):
    """(dense map users, clusters, position of the stray entry that gets an id above every user): file order matters -- user 7 first
    with one cluster, at the end with another; a negative id in the middle."""
    named = np.setdiff1d(np.arange(1, FLAT_U + 1), FLAT_UNMAPPED)
    cl = (named * 5 + 1) % K
    first = int(np.flatnonzero(named == FLAT_TWICE)[0])
    mu = np.r_[named[:20], -3, named[20:], 0, FLAT_TWICE]        # the 0 is a placeholder for the id above max_user
    mc = np.r_[cl[:20], 1 % K, cl[20:], 2 % K, (cl[first] + 1) % K]
    assert len(mu) == FLAT_N_MAP
    return mu.astype(np.int64), mc.astype(np.int32), 21 + len(named) - 20


def flat_map_last_wins(K):
    """the same map as the oracle gets it: one pair per user, the last; no stray entries"""
    mu, mc, stray = flat_map(K)
    cl = {}
    for k, (a, b) in enumerate(zip(mu.tolist(), mc.tolist())):
        if k != stray and a > 0:
            cl[a] = b
    users = np.array(sorted(cl), dtype=np.int32)
    return users, np.array([cl[int(x)] for x in users], dtype=np.int32)


FLAT_PATTERNS = rip.patterns(FLAT_U, FLAT_I, FLAT_N_MAP)


@functools.lru_cache(maxsize=None)
def flat_job(name, K, packed=None):
    """the flat job under one pattern, in a context of its own, mapped back to dense ids: (rows, sums, counters)"""
    P = pkg()
    f, g = FLAT_PATTERNS[name]
    u, i, s = rip.relabel_triples(flat_data(), f, g)
    mu, mc, stray = flat_map(K)
    ru = mu.copy()
    ru[mu > 0] = rip.relabel(mu[mu > 0], f)
    ru[stray] = int(f[-1]) + 9 if int(f[-1]) + 9 <= INT32_MAX else -11          # above every user where int32 has such an id
    conf = P.Configuration()
    conf.setFloat("lambda", FLAT_LAM)
    conf.setInt("numberOfItems", FLAT_I)
    conf.setInt("numberOfClusters", K)
    conf.setInt("numberOfRecommendations", FLAT_TOP)
    with environment({} if packed is None else {"FY_PREP_PACKED": packed}):
        ctx = P.Context(0)
        try:
            rec = P.RM2Job(conf, ctx).run((u, i, s), clustering=(ru.astype(np.int32), mc))
            out = rip.map_back(copy_of(rec.rows()), f, g), rip.map_back(copy_of(rec.sums()), f, g), counters(rec.stats)
            rec.close()
        finally:
            ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def flat_oracle(K):
    u, i, s = flat_data()
    mu, mc = flat_map_last_wins(K)
    return oracle.rm2(u, i, s, lam=FLAT_LAM, number_of_items=FLAT_I, number_of_recommendations=1 << 30, number_of_clusters=K,
                      map_user=mu, map_cluster=mc)


def check_flat_dense(K):
    rows, sums, st = flat_job("dense", K)
    ref = flat_oracle(K)
    assert_topn_matches(rows, ref, FLAT_TOP)
    assert np.array_equal(sums["user_id"], ref["user_id"]) and np.array_equal(sums["item_id"], ref["item_id"])
    np.testing.assert_array_equal(sums["user_sum"], ref["user_sum"])                      # (the bounds of tests/test_rm2_gpu.py)
    np.testing.assert_allclose(sums["item_coll"], ref["item_coll"], rtol=1e-14)
    # the map's cases really occur: the unmapped users sit in cluster 0, user 7 in its LATER cluster, more than one cluster is used
    by_user = dict(zip(rows["user"].tolist(), rows["cluster"].tolist()))
    mu, mc, _ = flat_map(K)
    assert all(by_user[x] == 0 for x in FLAT_UNMAPPED) and by_user[FLAT_TWICE] == int(mc[-1])
    assert st["n_users"] == FLAT_U and st["n_items"] == FLAT_I and st["n_clusters_nonempty"] == K
    return rows, sums, st


@pytest.mark.parametrize("name", sorted(FLAT_PATTERNS))
def test_flat_job_under_every_pattern(name):
    """K = 3.  dense against the oracle (which gets the map de-duplicated "last wins"); every pattern against dense as bytes."""
    want = check_flat_dense(3)
    got = flat_job(name, 3)
    for a, b in zip(got, want):
        assert_same_bytes(a, b)


# pack_edge_64 / 65: ib0 + ub0 + 16 = 64 / 65 with K = 1; pack_edge_k_*: the same sum 63 / 64 and one cluster bit with K = 2;
# int32_user_packed: user id 2^31 - 1 beside 16-bit items, 16 + 32 + 16 = 64 -- the packed mode at its widest user field
@pytest.mark.parametrize("name,K", [("pack_edge_64", 1), ("pack_edge_65", 1), ("pack_edge_k_64", 2), ("pack_edge_k_65", 2),
                                    ("int32_user_packed", 1), ("int32_edge", 1)])
def test_packed_gate(name, K):
    """Both sides of the packed gate, each with FY_PREP_PACKED=1 and 0, against dense in both modes: all four runs equal as bytes."""
    max_user, max_item = int(FLAT_PATTERNS[name][0][-1]), int(FLAT_PATTERNS[name][1][-1])
    assert rip.packed_gate(max_user, max_item, K) == (name in ("pack_edge_64", "pack_edge_k_64", "int32_user_packed"))
    want = check_flat_dense(K)
    for run in (flat_job("dense", K, "0"), flat_job(name, K, "1"), flat_job(name, K, "0")):
        for a, b in zip(run, want):
            assert_same_bytes(a, b)


# ------------------------------------------------------------------------------------------------ RM2, pruned flow and panel mode
WALK_PATTERNS = rip.patterns(WALK_USERS, WALK_ITEMS, WALK_USERS)
PRUNED = {"FY_COOC_MAX_CH": "256"}
PANEL = {"FY_COOC_MAX_CH": "256", "FY_PANEL_MIN_CLUSTERS": "1", "FY_PANEL_COLS": "256"}
REFINE = {"FY_COOC_MAX_CH": "256", "FY_SEED_CHUNKS": "2", "FY_REFINE_C": "1000"}


def register(name):
    """the 700-item data of test_score_walk_gpu under a pattern, registered the way test_cooc_rect_gpu registers DATA["exact"]"""
    key = "raw_ids:" + name
    if key not in EPI.DATA:
        f, g = WALK_PATTERNS[name]
        EPI.DATA[key] = (lambda: rip.relabel_triples(walk_dataset(False), f, g), WALK_ITEMS)
    return key


def walk_job(name, env, top_n=10):
    if name == "dense":
        return EPI.run("small", env, top_n)
    f, g = WALK_PATTERNS[name]
    rows, sums, st = EPI.run(register(name), env, top_n)
    return rip.map_back(rows, f, g), rip.map_back(sums, f, g), st


@pytest.mark.parametrize("mode", ["pruned", "panel"])
@pytest.mark.parametrize("name", ["netflix_like", "pack_edge_64", "int32_edge"])
def test_pruned_flow_and_panel_mode(name, mode):
    env = PRUNED if mode == "pruned" else PANEL
    r0, s0, st0 = walk_job("dense", env)
    r1, s1, st1 = walk_job(name, env)
    print(name, mode, {k: (st0[k], st1[k]) for k in EPI.STATS + ("panel_clusters",)})
    for st in (st0, st1):
        assert st["blocks_total"] > 0 and st["prune_fallbacks"] == 0
        assert (st["panel_clusters"] > 0) == (mode == "panel")
    assert_topn_matches(r0, walk_reference(False, EPI.LAM), 10)
    assert_same_bytes(r1, r0)
    assert_same_bytes(s1, s0)
    assert_same_bytes(counters(st1), counters(st0))


def test_refinement_gate():
    """max_item = 2^28 - 1: the pass runs (through a 1 GiB raw-id table) and gives the dense job's bytes; 2^28 and 2^31 - 1: it is switched
    off -- rows_refined == 0, and the rows are the oracle's -- instead of indexing a truncated table."""
    ref = walk_reference(False, EPI.LAM)
    r0, s0, st0 = walk_job("dense", REFINE, 100)
    r1, s1, st1 = walk_job("refine_edge_on", REFINE, 100)
    print("rows refined", st0["rows_refined"], st1["rows_refined"])
    assert st0["rows_refined"] > 0 and st1["rows_refined"] == st0["rows_refined"] and st0["blocks_total"] > 0
    assert_topn_matches(r0, ref, 100)
    assert_same_bytes(r1, r0)
    assert_same_bytes(s1, s0)
    for name in ("refine_edge_off", "int32_edge"):
        r2, s2, st2 = walk_job(name, REFINE, 100)
        assert st2["rows_refined"] == 0 and st2["blocks_total"] > 0, name
        assert_topn_matches(r2, ref, 100, rtol=RTOL)
        assert_same_bytes(s2, s0)


# ------------------------------------------------------------------------------------------------ RM2 on request
@pytest.mark.parametrize("name", ["int32_edge", "netflix_like"])
def test_request_for_users_at_the_extremes(name):
    """score_users with request ids that ARE in the data at both ends of the range (0 and 2^31 - 1 under int32_edge), some twice, and ids
    that are not: the oracle's rows of those users (as test_rm2_request_gpu compares), and the dense request's bytes."""
    P = pkg()
    K = 3
    dense_ids = np.array([1, FLAT_U, 2, 25, FLAT_TWICE, 5, FLAT_U, 1], dtype=np.int64)
    ref = flat_oracle(K)
    keep = np.isin(ref["rec_user"], dense_ids)
    exp = {k: ref[k][keep] for k in ("rec_user", "rec_item", "rec_score", "rec_cluster")}
    mu, mc = flat_map_last_wins(K)
    answers = []
    for pattern in ("dense", name):
        f, g = FLAT_PATTERNS[pattern]
        u, i, s = rip.relabel_triples(flat_data(), f, g)
        ids = rip.relabel(dense_ids, f)
        if pattern == "int32_edge":
            assert ids.min() == 0 and ids.max() == INT32_MAX
        absent = np.setdiff1d(np.array([int(f[0]) + 1, int(f[-1]) - 1, -1, -(2 ** 31)]), f)      # neighbours of the extremes, not in the data
        conf = P.Configuration()
        conf.setFloat("lambda", FLAT_LAM)
        conf.setInt("numberOfItems", FLAT_I)
        conf.setInt("numberOfClusters", K)
        conf.setInt("numberOfRecommendations", FLAT_TOP)
        ctx = P.Context(0)
        try:
            job = P.RM2Job(conf, ctx).prepare((u, i, s), clustering=(rip.relabel(mu, f), mc))
            rec = job.score_users(np.r_[ids, absent].astype(np.int32))
            rows = rip.map_back(copy_of(rec.rows()), f, g)
            assert rec.stats["users_scored"] == len(np.unique(dense_ids)) and rec.request_stats is not None
            rec.close()
            job.close()
        finally:
            ctx.close()
        assert_topn_matches(rows, exp, FLAT_TOP, rtol=RTOL)
        answers.append(rows)
    assert_same_bytes(answers[1], answers[0])


# ------------------------------------------------------------------------------------------------ item similarity
SIM_U, SIM_I, SIM_K = 150, 300, 20
SIM_PATTERNS = rip.patterns(SIM_U, SIM_I, 0)
SIM_ASKED = np.array([1, SIM_I, 2, 150, 299, SIM_I, 17], dtype=np.int64)      # both extremes, one twice


@functools.lru_cache(maxsize=None)
def sim_data():
    return half_star_data(SIM_U, SIM_I, 0.08, 20261022)


def sim_runs(ctx, name, measure):
    """(full build, rows of SIM_ASKED from a prepared job), mapped back"""
    P = pkg()
    f, g = SIM_PATTERNS[name]
    triples = rip.relabel_triples(sim_data(), f, g)
    full = P.RowSimilarityJob(ctx).run(triples, similarityClassname=measure, maxSimilaritiesPerRow=SIM_K)
    job = P.RowSimilarityJob(ctx).prepare(triples, similarityClassname=measure, maxSimilaritiesPerRow=SIM_K)
    try:
        asked = job.rows(np.r_[rip.relabel(SIM_ASKED, g), -1].astype(np.int32))
        assert asked.request_stats["items_known"] == len(np.unique(SIM_ASKED))
        return rip.map_back(copy_of(full.rows()), f, g), rip.map_back(copy_of(asked.rows()), f, g), counters(full.stats)
    finally:
        job.close()


@pytest.mark.parametrize("gram", ["0", "1"])
@pytest.mark.parametrize("measure", [MR.COSINE, MR.TANIMOTO])
def test_item_similarity(monkeypatch, measure, gram):
    """Row-at-a-time and symmetric build, the whole matrix and the rows of named items: dense against the statement, patterns against
    dense as bytes."""
    monkeypatch.setenv("FY_ISIM_GRAM", gram)
    ctx = pkg().Context(0)
    try:
        u, i, s = sim_data()
        full0, asked0, st0 = sim_runs(ctx, "dense", measure)
        info = MR.check_rows(full0, u, i, s, measure, SIM_K)
        print(measure, gram, info)
        assert info["rows"] > 0 and (gram == "0" or st0["isim_candidates"] > 0)
        MR.check_rows(asked0, u, i, s, measure, SIM_K, only_items=np.unique(SIM_ASKED))
        assert set(asked0["item"].tolist()) == set(SIM_ASKED.tolist())
        for name in ("zero_based", "netflix_like", "pow2_item_lo", "pow2_item_hi", "int32_edge"):
            full1, asked1, st1 = sim_runs(ctx, name, measure)
            assert_same_bytes(full1, full0)
            assert_same_bytes(asked1, asked0)
            # (how many candidates the symmetric build's sweep appends depends on when a row's rising threshold reaches the other
            # workgroups -- fy_itemsim.hip, sweep_take -- and differs between two runs of one input: every other counter is compared)
            timing = ("isim_candidates", "isim_redone_rows")
            assert_same_bytes({k: v for k, v in st1.items() if k not in timing}, {k: v for k, v in st0.items() if k not in timing})
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ item-based CF
CF_USERS = np.array([1, SIM_U, 3, 77], dtype=np.int64)
CF_ITEMS = np.r_[1, SIM_I, np.arange(2, SIM_I, 3)].astype(np.int64)


def cf_runs(ctx, name):
    P = pkg()
    f, g = SIM_PATTERNS[name]
    triples = rip.relabel_triples(sim_data(), f, g)
    job = P.BaselineRecommenderJob(ctx)
    rec, sims = job.run(triples, numRecommendations=10, maxPrefsPerUser=12, maxSimilaritiesPerItem=SIM_K)
    users, items = rip.relabel(CF_USERS, f), rip.relabel(CF_ITEMS, g)
    some, _ = job.run(triples, numRecommendations=10, maxPrefsPerUser=12, maxSimilaritiesPerItem=SIM_K, similarities=sims,
                      usersFile=users, itemsFile=items)
    prepared = job.prepare(triples, maxSimilaritiesPerItem=SIM_K)
    try:
        asked = prepared.recommend(users, numRecommendations=10, maxPrefsPerUser=12, itemsFile=items)
        out = {"all": rec.rows(), "filtered": some.rows(), "prepared": asked.rows(), "sims": sims.rows(), "pairs": sims.pairs()}
        return {k: rip.map_back(copy_of(v), f, g) for k, v in out.items()}
    finally:
        prepared.close()


@pytest.mark.parametrize("name", ["netflix_like", "int32_edge"])
def test_item_based_cf(name):
    ctx = pkg().Context(0)
    try:
        u, i, s = sim_data()
        d = cf_runs(ctx, "dense")
        ref = oracle.itemcf(u, i, s, d["sims"]["item"], d["sims"]["other"], d["sims"]["sim"].astype(np.float64), num_recommendations=1 << 30,
                            max_prefs_per_user=12)
        ICF.check(d["all"], ref, 10)
        # the filtered lists: the requested users' candidates among the allowed items, in the oracle's order
        keep = np.isin(ref["user"], CF_USERS) & np.isin(ref["item"], CF_ITEMS)
        only = {k: ref[k][keep] for k in ("user", "item", "score")}
        assert len(d["filtered"]["user"]) > 0 and set(d["filtered"]["user"].tolist()) <= set(CF_USERS.tolist())
        ICF.check(d["filtered"], only, 10)
        ICF.check(d["prepared"], only, 10)
        # pairs(): a = min id, b = max id, every unordered pair of the rows once
        pairs = d["pairs"]
        assert np.all(pairs["a"] < pairs["b"]) and len(pairs["a"]) > 0
        lo, hi = np.minimum(d["sims"]["item"], d["sims"]["other"]), np.maximum(d["sims"]["item"], d["sims"]["other"])
        assert set(zip(pairs["a"].tolist(), pairs["b"].tolist())) == set(zip(lo.tolist(), hi.tolist()))
        assert pairs["a"].min() == 1 and pairs["b"].max() == SIM_I, "no pair with an item at either extreme"
        r = cf_runs(ctx, name)
        for k in d:
            assert_same_bytes(r[k], d[k])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the sharded prep's gate
def device_doubles(ptr, n):
    import torch
    par = __import__("importlib").import_module("filmyou-core_amd.parallel")
    return torch.as_tensor(par._DevicePointer(ptr, n, "<f8"), device="cuda:0")


@pytest.mark.parametrize("name", ["shard_edge_on", "shard_edge_off"])
def test_sharded_prep_gate(name):
    """The one-GPU rehearsal of test_multirank_gpu.sharded_equals_single, K = 4, two ranks, nRU + nRI = 2^25 and 2^25 + 1: the exchange
    buffer is laid out by raw id exactly in the first case, and both agree with the single-rank job row for row (half stars: the item
    statistics are sums of exact values in any order, hence the same bits)."""
    import torch
    P = pkg()
    K, world = 4, 2
    f, g = FLAT_PATTERNS[name]
    max_user, max_item = int(f[-1]), int(g[-1])
    u, i, s = rip.relabel_triples(flat_data(), f, g)
    uu = np.unique(u)
    clustering = (uu, (np.arange(len(uu)) % K).astype(np.int32))
    conf = P.Configuration()
    conf.setFloat("lambda", FLAT_LAM)
    conf.setInt("numberOfItems", FLAT_I)
    conf.setInt("numberOfClusters", K)
    conf.setInt("numberOfRecommendations", FLAT_TOP)
    ctx = P.Context(0)
    try:
        ratings = P.Ratings(ctx, u, i, s)
        job = P.RM2Job(conf, ctx)
        single = job.run(ratings, clustering=clustering)
        prepared = [job.prepare(ratings, clustering=clustering, rank=r, world=world) for r in range(world)]
        layouts = {pr.stats_layout() for pr in prepared}
        assert len(layouts) == 1
        n_item_slots, n_user_slots = layouts.pop()
        print(name, "layout", n_item_slots, n_user_slots)
        assert (n_user_slots > 0) == rip.sharded_prep_allowed(max_user, max_item) == (name == "shard_edge_on")
        if n_user_slots:
            assert (n_item_slots, n_user_slots) == (max_item + 1, max_user + 1)
        else:
            assert n_item_slots == FLAT_I
        parts = []
        for pr in prepared:
            ptr, n = pr.partial_stats()
            parts.append(device_doubles(ptr, n).clone())
        torch.cuda.synchronize()
        gathered = torch.cat(parts).contiguous()
        torch.cuda.synchronize()        # half a gigabyte on torch's stream; the library reads it on its own, which waits for nobody
        results = []
        for pr in prepared:
            pr.set_global_stats(gathered.data_ptr())
            results.append(pr.score())
            pr.close()
        for r in results:
            assert_same_bytes(copy_of(r.sums()), copy_of(single.sums()))
        rows = {k: np.concatenate([r.rows()[k] for r in results]) for k in ("user", "item", "score", "cluster")}
        order = lambda r: np.lexsort((r["item"], r["user"]))
        a, b = order(rows), order(single.rows())
        assert_same_bytes({k: v[a] for k, v in rows.items()}, {k: single.rows()[k][b] for k in rows})
        # and the single-rank job on these ids is the dense job, which is the oracle's
        back = rip.map_back(copy_of(single.rows()), f, g)
        ref = oracle.rm2(*flat_data(), lam=FLAT_LAM, number_of_items=FLAT_I, number_of_recommendations=1 << 30, number_of_clusters=K,
                         map_user=np.arange(1, FLAT_U + 1, dtype=np.int32), map_cluster=clustering[1])
        assert_topn_matches(back, ref, FLAT_TOP)
        ratings.close()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ sub-cluster mappings, refinement
def test_sub_cluster_mappings_and_refinement_under_netflix_like_ids():
    """These tables are sized by raw id: netflix_like only.  The restatement of tests/refine_ref.py works on raw ids, so it is run on the
    relabelled input itself."""
    import test_refine_gpu as TR
    P = pkg()
    ctx = P.Context(0)
    try:
        (u, i, s), mu, mc, K = TR.ragged_mapping_input(1)
        pat = rip.patterns(int(mu.max()), int(i.max()), len(mu))["netflix_like"]
        f, g = pat
        ru, ri, rmu = rip.relabel(u, f), rip.relabel(i, g), rip.relabel(mu, f)
        got = P.SubClusterMappingJob(TR.conf_of(numberOfClusters=K), ctx).run((ru, ri, s), (rmu, mc))
        m = RR.mappings(ru, ri, s, rmu, mc, K)
        assert got.user.tolist() == np.concatenate(m["users"]).tolist() and got.user.max() == 2649429
        assert got.item.tolist() == np.concatenate(m["items"]).tolist()
        assert got.users_in_cluster.tolist() == [len(x) for x in m["users"]] and got.items_in_cluster.tolist() == [len(x) for x in m["items"]]
        assert got.user_new_id.tolist() == np.concatenate([np.arange(1, len(x) + 1) for x in m["users"]]).tolist()
        assert got.item_new_id.tolist() == np.concatenate([np.arange(1, len(x) + 1) for x in m["items"]]).tolist()
        assert got.nnz == int(m["kept"].sum())
        vals = s[m["kept"]]
        for have, want in ((got.csr, RR.csr(m["row_user"], m["row_item"], vals, len(got.user))),
                           (got.csc, RR.csr(m["row_item"], m["row_user"], vals, len(got.item)))):
            for a, b in zip(have, want):
                assert np.array_equal(a, b)
        # the refinement itself: 40 users x 25 items in two parents, against the composed oracles on the same raw ids
        su, si, ss, users = TR.small_input()
        f2, g2 = rip.patterns(40, 25, 40)["netflix_like"]
        su, si, users = rip.relabel(su, f2), rip.relabel(si, g2), rip.relabel(users, f2)
        cl = (np.arange(40) % 2).astype(np.int32)
        m2 = RR.mappings(su, si, ss, users, cl, 2)
        kc = RR.sub_clusters(m2, 5)
        H0, W0 = RR.seeded_initial(m2, kc, 5)
        ou, oc, ocount, _, ties, _ = RR.composed_refinement(su, si, ss, users, cl, 2, 5, 60, 4, True, 2, H0, W0)
        job = P.ClusterRefinementJob(TR.conf_of(numberOfUsers=60, numberOfClusters=2, usersPerSubCluster=5, numberOfIterations=4,
                                                normalizationFrequency=2), ctx)
        got_u, got_c, counts = job.run((su, si, ss), (users, cl), seed=5)
        assert got_u.tolist() == ou.tolist() and got_u.max() == 2649429
        differ = got_c != oc
        assert ties.sum() <= 0.001 * len(got_u) and not (differ & ~ties).any()
        assert np.array_equal(np.bincount(got_c, minlength=len(counts)), counts)
    finally:
        ctx.close()


def rip_conf(K):
    c = pkg().Configuration()
    c.setInt("numberOfClusters", K)
    return c


def test_refinement_refuses_the_ids_its_tables_cannot_hold():
    """User id 2^31 - 1 (the user table has max id + 1 entries) and item id 2^31 - 1 (numberOfClusters x (max item id + 1) slots) are
    FY_ERR_UNSUPPORTED before any table is sized, and the context runs a job afterwards."""
    import test_refine_gpu as TR
    P = pkg()
    ctx = P.Context(0)
    try:
        u = np.array([1, 2, INT32_MAX], np.int32)
        i = np.array([1, 2, 2], np.int32)
        s = np.ones(3, np.float32)
        cl = np.array([0, 1, 1], np.int32)
        refine = P.ClusterRefinementJob(TR.conf_of(numberOfUsers=3, numberOfClusters=2, usersPerSubCluster=2, numberOfIterations=1), ctx)
        for run in (lambda: refine.run((u, i, s), (u, cl)),                                   # fy_cluster_refine, user id 2^31 - 1
                    lambda: P.SubClusterMappingJob(rip_conf(2), ctx).run((u, i, s), (u, cl)),  # fy_submap_create, the same
                    lambda: P.SubClusterMappingJob(rip_conf(2), ctx).run((i, u, s), (i, cl))):  # item id 2^31 - 1
            with pytest.raises(RuntimeError) as e:
                run()
            assert e.value.__cause__.code == FY_ERR_UNSUPPORTED, str(e.value)
        got = P.SubClusterMappingJob(rip_conf(2), ctx).run((i, i, s), (np.array([1, 2], np.int32), np.array([0, 1], np.int32)))
        assert got.user.tolist() == [1, 2]
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ errors
@pytest.mark.parametrize("packed", ["0", "1"])
def test_errors_beside_the_largest_ids(monkeypatch, packed):
    monkeypatch.setenv("FY_PREP_PACKED", packed)
    P = pkg()
    f, g = FLAT_PATTERNS["int32_edge"]
    u, i, s = rip.relabel_triples(flat_data(), f, g)
    conf = P.Configuration()
    conf.setFloat("lambda", FLAT_LAM)
    conf.setInt("numberOfItems", FLAT_I)
    conf.setInt("numberOfClusters", 1)
    ctx = P.Context(0)
    try:
        for bad_u, bad_i in ((-1, 5), (5, -1), (-(2 ** 31), INT32_MAX)):
            with pytest.raises(RuntimeError, match="negative user or item id") as e:
                P.RM2Job(conf, ctx).run((np.r_[u, bad_u].astype(np.int32), np.r_[i, bad_i].astype(np.int32), np.r_[s, np.float32(2.5)]))
            assert e.value.__cause__.code == FY_ERR_NEGATIVE_ID
        has = bool(np.any((u == INT32_MAX) & (i == INT32_MAX)))
        du = np.r_[u, INT32_MAX, INT32_MAX][: len(u) + (1 if has else 2)].astype(np.int32)
        di = np.r_[i, INT32_MAX, INT32_MAX][: len(du)].astype(np.int32)
        ds = np.r_[s, np.float32(1.5), np.float32(4.0)][: len(du)]
        with pytest.raises(RuntimeError, match=r"share one \(user, item\) key") as e:
            P.RM2Job(conf, ctx).run((du, di, ds))
        assert e.value.__cause__.code == FY_ERR_DUPLICATE_RATING
        rec = P.RM2Job(conf, ctx).run((u, i, s))          # the context still runs a job
        assert rec.stats["n_users"] == FLAT_U
    finally:
        ctx.close()
