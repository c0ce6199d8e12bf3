"""The two epilogues of the RM2 row kernel (FY_COOC_EPI, fy_rm2.hip: cooc_rm2_epilogue_pack) store the same matrix and the same block maxima,
and the two lane exchanges of k_topn_seed's register sort (FY_TOPN_SEED_XL) give the same lists.

FY_COOC_EPI=1 converts, packs and stores eight columns per lane for the plain 24-bit items -- a half-wave is one 256-column block -- and takes
every block maximum without LDS; FY_COOC_EPI=0 is the loop it replaces.  Every element goes through the same roundings and a maximum has no
order, so the outputs must be equal byte for byte.  The matrix and Bmax are not outputs of a job; they show through it:

  * a wrong matrix element changes a score: rows() and sums() of the two epilogues are compared as bytes;
  * a block maximum that came out too LARGE changes no list, only the work: blocks_total, blocks_survived, log_terms_evaluated, bound_repairs and
    prune_fallbacks of the two epilogues must be equal (the padding columns behind the last item belong to the last block: a value left in them
    shows the same way);
  * a block maximum that came out too SMALL drops a block somebody needs: the pruned flow must equal the full pass (FY_PRUNE=0) byte for byte.

Where the eight-column loop can go wrong is at the ends of an item: a half-wave at or behind the item's last block (an odd number of blocks), an
item of one block, a second trip with one wave in it, a row's own chunk, which starts at the row's diagonal block.  Shapes: (a) 700 items in one
chunk of three blocks (rows in block 0 / 1 / 2 leave three, two, one); (b) the same with chunks of one and of two blocks; (c) 2 400 items, ten
blocks, a workgroup of four waves (2 048 columns a trip: two trips, the second with one wave), and with chunks of three blocks; (d) the linear
accumulator layout and the fp64 accumulators.  One cluster, half-star ratings, an item's column is its popularity rank.
"""
import functools
import os

import numpy as np
import pytest

from test_score_walk_gpu import N_ITEMS, dataset, reference
from util import assert_topn_matches, pkg

pytestmark = pytest.mark.gpu

ENV = {"FY_M24_MIN_ITEMS": "0", "FY_PRUNE_MIN_ITEMS": "256", "FY_PRUNE_MIN_USERS": "1", "FY_SEED_CHUNKS": "1"}
STATS = ("blocks_total", "blocks_survived", "log_terms_evaluated", "bound_repairs", "prune_fallbacks")
LAM = "0.1"
WIDE_USERS, WIDE_ITEMS = 600, 2400


@functools.lru_cache(maxsize=None)
def wide_dataset():
    """600 users x 2 400 items by the recipe of test_score_walk_gpu.dataset: the 256 seed columns popular (200 ... 100 raters), the rest with
    30 ... 10, 45 % of an item's raters from a group of 104 users with short lists -- the bounds then cut seven blocks of eight and the batch
    does not fall back to the full pass, so the lists really depend on Bmax.  The set is also dense enough (more pair visits, sum of n_u^2,
    than the matrix has elements) for its FY_PRUNE=0 job to keep the symmetric walk.  (A first, sparser set -- 80 ... 40 and 8 ... 3 raters,
    users drawn uniformly, 1.2 M pair visits for 5.8 M elements -- fell back, and its FY_PRUNE=0 job takes the full-row walk of
    FY_FULL_WALK_SPARSE, whose scores differ from the symmetric walk's in the last bit of some rows
    (profiles/rm2_smoothing/pruned_vs_unpruned_bits.txt): 93 of 6 000 here, with either epilogue, and in the commit before this test as well.
    That difference is not the epilogue's and is not what this file is about.)"""
    rng = np.random.default_rng(20261019)
    cols = np.arange(WIDE_ITEMS)
    target = np.where(cols < 256, 100 + (255 - cols) * 100 // 255, 10 + (WIDE_ITEMS - 1 - cols) * 20 // (WIDE_ITEMS - 257))
    group_b, group_a = np.arange(0, 104), np.arange(104, WIDE_USERS)
    w_a, w_b = rng.uniform(0.7, 1.6, len(group_a)), rng.uniform(0.5, 1.5, len(group_b))
    users = []
    for j in range(WIDE_ITEMS):
        nb = int(round(target[j] * 0.45))
        users.append(rng.choice(group_b, nb, replace=False, p=w_b / w_b.sum()))
        users.append(rng.choice(group_a, int(target[j]) - nb, replace=False, p=w_a / w_a.sum()))
    user = np.concatenate(users).astype(np.int32) + 1
    col = np.repeat(cols, target).astype(np.int32)
    assert len(np.unique(user)) == WIDE_USERS
    score = (0.5 * (1 + (user.astype(np.int64) * 7 + col.astype(np.int64) * 13) % 10)).astype(np.float32)
    return user, col + 1, score


DATA = {"small": (lambda: dataset(False), N_ITEMS), "wide": (wide_dataset, WIDE_ITEMS)}


@functools.lru_cache(maxsize=None)
def job(data, top_n, env):
    """One job in a context of its own (the library reads FY_* when the context is created); `env` = sorted (name, value) pairs beside ENV.
    Cached: the tests share their runs.  Returns copies: rows, side outputs, stats."""
    P = pkg()
    want = {**ENV, **dict(env)}
    saved = {k: os.environ.get(k) for k in want}
    os.environ.update(want)
    try:
        (u, i, s), n_items = DATA[data][0](), DATA[data][1]
        uu = np.unique(u)
        conf = P.Configuration()
        conf.set("lambda", LAM)
        conf.setInt("numberOfItems", n_items)
        conf.setInt("numberOfClusters", 1)
        conf.setInt("numberOfRecommendations", top_n)
        ctx = P.Context(0)
        rec = P.RM2Job(conf, ctx).run((u, i, s), clustering=(uu, np.zeros(len(uu), dtype=np.int32)))
        rows = {k: np.array(v, copy=True) for k, v in rec.rows().items()}
        sums = {k: np.array(v, copy=True) for k, v in rec.sums().items()}
        stats = dict(rec.stats)
        rec.close()
        ctx.close()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return rows, sums, stats


def run(data, env, top_n=10):
    return job(data, top_n, tuple(sorted(env.items())))


def assert_same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), k


def check_epilogues(data, env):
    """Old against new epilogue, and the new build's pruned flow against its full pass.  Returns the new epilogue's rows."""
    r0, s0, st0 = run(data, {**env, "FY_COOC_EPI": "0"})
    r1, s1, st1 = run(data, {**env, "FY_COOC_EPI": "1"})
    rf, sf, stf = run(data, {**env, "FY_COOC_EPI": "1", "FY_PRUNE": "0"})
    print({k: (st0[k], st1[k]) for k in STATS})
    assert len(r1["user"]) > 0
    assert_same_bytes(r0, r1)
    assert_same_bytes(s0, s1)
    for k in STATS:
        assert st0[k] == st1[k], k
    assert st1["blocks_total"] > 0, "the branch and bound did not run: nobody read Bmax"
    assert stf["blocks_total"] == 0
    assert_same_bytes(r1, rf)
    assert_same_bytes(s1, sf)
    return r1, st1


def test_one_chunk_of_three_blocks():
    """(a) CH = 704, c1 = ldm = 768: the second wave's upper half is masked; rows of the three diagonal blocks leave 3, 2, 1 blocks."""
    rows, st = check_epilogues("small", {})
    assert st["prune_fallbacks"] == 0 and st["blocks_survived"] > 0
    assert_topn_matches(rows, reference(False, LAM), 10)      # the tolerance of every forced 24-bit job: relative 1e-5


@pytest.mark.parametrize("max_ch", ["256", "512"])
def test_chunks_of_one_and_two_blocks(max_ch):
    """(b) items of a lone half-wave; a row's own chunk and the chunks behind it."""
    check_epilogues("small", {"FY_COOC_MAX_CH": max_ch})


@pytest.mark.parametrize("env", [{}, {"FY_COOC_MAX_CH": "768"}], ids=["ten_blocks", "chunks_of_three_blocks"])
def test_two_trips_of_four_waves(env):
    """(c) ldm = 2560, four waves: a second trip with one active wave; rows of the ninth and tenth block leave two and one.  Chunks of 768
    columns: a masked trailing half-wave in every full item."""
    _, st = check_epilogues("wide", {"FY_COOC_BLOCK": "256", **env})
    assert st["prune_fallbacks"] == 0 and st["blocks_survived"] > 0


@pytest.mark.parametrize("env", [{"FY_COOC_PLANES": "0"}, {"FY_COOC_FX": "0"}], ids=["linear_layout", "fp64_accumulators"])
def test_other_accumulators(env):
    """(d) the linear layout keeps four columns per lane, the fp64 accumulators take eight: the same bytes under both switches, and the same
    lists as the default job's within the oracle's tolerance."""
    rows, _ = check_epilogues("small", env)
    assert_topn_matches(rows, reference(False, LAM), 10)


@pytest.mark.parametrize("top_n,seed_chunks", [(10, "1"), (100, "2")], ids=["seed_256", "seed_512"])
def test_seed_sort_exchanges_give_the_same_lists(top_n, seed_chunks):
    """(e) k_topn_seed<4> sorts the 256 seed columns of FY_SEED_CHUNKS=1; lists of 100 over two seed chunks (what a list of 100 takes by
    default; forced here like the first) are sorted by k_topn_seed<8>.  Lane exchanges by DPP / v_permlane swaps against __shfl_xor."""
    env = {"FY_SEED_CHUNKS": seed_chunks}
    r0, s0, st0 = run("small", {**env, "FY_TOPN_SEED_XL": "0"}, top_n)
    r1, s1, st1 = run("small", {**env, "FY_TOPN_SEED_XL": "1"}, top_n)
    assert st1["blocks_total"] > 0, "the pruned flow did not run: nobody sorted a seed"
    assert_same_bytes(r0, r1)
    assert_same_bytes(s0, s1)
    for k in STATS:
        assert st0[k] == st1[k], k
    assert_topn_matches(r1, reference(False, LAM), top_n)
