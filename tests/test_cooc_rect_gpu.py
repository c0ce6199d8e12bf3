"""The two orientations of the symmetric row walk (FY_COOC_RECT, CoocArgs::half 1 / 2).

FY_COOC_RECT=0: row i of chunk c stores its own chunk from its diagonal block on and the chunks BEHIND it.  FY_COOC_RECT=1 (the default): its
own chunk likewise and the WHOLE chunks IN FRONT of it -- the off-diagonal chunk rectangles are accumulated from the side of the unpopular
rows.  Item list, segment tables, the epilogue's block maxima, the three mirror passes and the refinement pass's copies all follow one
predicate (cooc_tile_stored).  A contribution to G[i][j] is one fp32 rounding of W_vi r_vj on one side and of W_vj r_vi on the other, so the
two matrices may differ in the last bit inside the rectangles and nowhere else:

  * rows of both orientations match the CPU oracle within RTOL, and the side outputs (which do not depend on G) are equal as bytes;
  * under RECT=1 the pruned flow equals the full pass (FY_PRUNE=0) byte for byte: a block maximum that is too SMALL drops a needed block;
    prune_fallbacks == 0 and blocks_survived > 0, so Bmax was read;
  * FY_LAZY_MIRROR=0 equals 1 byte for byte: the `need` path and the full mirror go through the same predicate;
  * a seed of two blocks with lists of 100 re-scores rows from the fp64 copies (head32 / tail32): rows_refined > 0 and the oracle's scores;
  * on a data set where NOTHING is rounded on either side (every user's ratings sum to a power of two) the two orientations agree byte for
    byte in rows, sums and the five pruning statistics: a block maximum that is too LARGE, or a tile mirrored to the wrong place, shows here.

Shapes: 700 items in three chunks of one block (every rectangle one tile, the own chunk the diagonal block alone) and in two chunks, the
last ragged; 2 400 items in four chunks of 768 (the last of 96 columns) and three of 1 024 (the last of 352), workgroups of four waves.
"""
import functools

import numpy as np
import pytest

import oracle
from test_cooc_epilogue_gpu import DATA, LAM, STATS, WIDE_ITEMS, assert_same_bytes, run, wide_dataset
from test_score_walk_gpu import reference
from util import assert_topn_matches

pytestmark = pytest.mark.gpu

SHAPES = {
    "small_3x256": ("small", {"FY_COOC_MAX_CH": "256"}),
    "small_512_188": ("small", {"FY_COOC_MAX_CH": "512"}),
    "wide_3x768_96": ("wide", {"FY_COOC_BLOCK": "256", "FY_COOC_MAX_CH": "768"}),
    "wide_2x1024_352": ("wide", {"FY_COOC_BLOCK": "256", "FY_COOC_MAX_CH": "1024"}),
}


def oracle_of(triples, n_items):
    u, i, s = triples
    uu = np.unique(u)
    return oracle.rm2(u, i, s, lam=float(LAM), number_of_items=n_items, number_of_recommendations=1 << 30, number_of_clusters=1,
                      map_user=uu, map_cluster=np.zeros(len(uu), dtype=np.int32), n_threads=8)


@functools.lru_cache(maxsize=None)
def wide_reference():
    return oracle_of(wide_dataset(), WIDE_ITEMS)


def reference_of(data):
    return reference(False, LAM) if data == "small" else wide_reference()


@functools.lru_cache(maxsize=None)
def exact_dataset():
    """wide_dataset with every user's ratings moved in half-star steps (inside 0.5 ... 5) until they sum to a power of two: one always lies
    in [0.5 n, 5 n].  Then r / s / s and its product with a half-star rating are exact in fp32 whichever side forms them."""
    user, item, score = wide_dataset()
    score = score.copy()
    order = np.argsort(user, kind="stable")
    bounds = np.flatnonzero(np.diff(user[order])) + 1
    for idx in np.split(order, bounds):
        half = np.rint(score[idx] * 2).astype(np.int64)               # ratings in half stars, 1 ... 10
        n, total = len(half), int(half.sum())
        powers = [p for p in (1 << k for k in range(1, 40)) if n <= p <= 10 * n]      # sums (in half stars) that are powers of two
        assert powers
        want = min(powers, key=lambda p: abs(p - total))
        step = 1 if want > total else -1
        k = 0
        while total != want:                                          # round robin, one half star at a time
            if 1 <= half[k % n] + step <= 10:
                half[k % n] += step
                total += step
            k += 1
        score[idx] = (half * 0.5).astype(np.float32)
    return user, item, score


DATA["exact"] = (exact_dataset, WIDE_ITEMS)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_both_orientations(shape):
    data, env = SHAPES[shape]
    r0, s0, st0 = run(data, {**env, "FY_COOC_RECT": "0"})
    r1, s1, st1 = run(data, {**env, "FY_COOC_RECT": "1"})
    rf, sf, stf = run(data, {**env, "FY_COOC_RECT": "1", "FY_PRUNE": "0"})
    rm, sm, stm = run(data, {**env, "FY_COOC_RECT": "1", "FY_LAZY_MIRROR": "0"})
    print(shape, {k: (st0[k], st1[k]) for k in STATS}, "segments", st0["cooc_segments"], st1["cooc_segments"])
    ref = reference_of(data)
    w0 = assert_topn_matches(r0, ref, 10)
    w1 = assert_topn_matches(r1, ref, 10)
    print(shape, "worst relative error against the oracle: RECT=0 %.3g, RECT=1 %.3g" % (w0, w1))
    assert_same_bytes(s0, s1)
    for st in (st0, st1, stm):
        assert st["prune_fallbacks"] == 0 and st["blocks_survived"] > 0 and st["blocks_total"] > 0, "the bounds did not bite: nobody needed Bmax"
    assert stf["blocks_total"] == 0
    assert_same_bytes(r1, rf)
    assert_same_bytes(s1, sf)
    assert_same_bytes(r1, rm)
    assert_same_bytes(s1, sm)
    for k in STATS:
        assert st1[k] == stm[k], k
    assert st1["cooc_segments"] != st0["cooc_segments"], "both runs took the same walk"


@pytest.mark.parametrize("max_ch", ["256", "512"])
def test_refinement_reads_the_tail_copies(max_ch):
    """Seed of 512 columns, lists of 100.  Chunks of 256: the head rows span two chunks (head32 holds their items in front of their own
    chunk, through the four-column loop); chunks of 512: the head rows are the first chunk and the rows behind it leave their 512 head
    columns in tail32 from the eight-column loop.  No score of this data set nearly cancels (rows_refined was 0 at the default threshold),
    so FY_REFINE_C is raised until every list row whose item is a head column is scored again from the copies: a copy read from the
    wrong place then shows against the oracle."""
    env = {"FY_COOC_MAX_CH": max_ch, "FY_SEED_CHUNKS": "2", "FY_REFINE_C": "1000"}
    r0, s0, st0 = run("small", {**env, "FY_COOC_RECT": "0"}, 100)
    r1, s1, st1 = run("small", {**env, "FY_COOC_RECT": "1"}, 100)
    print(max_ch, "rows refined", st0["rows_refined"], st1["rows_refined"])
    assert st1["rows_refined"] > 0 and st1["rows_refined"] == st0["rows_refined"]
    assert st1["blocks_total"] > 0
    ref = reference(False, LAM)
    assert_topn_matches(r0, ref, 100)
    assert_topn_matches(r1, ref, 100)
    assert_same_bytes(s0, s1)


def test_exact_products_give_the_same_bytes():
    """Nothing is rounded on either side, so the two walks build the same matrix to the bit: rows, sums and all five statistics."""
    user, _, score = exact_dataset()
    sums = np.bincount(user, weights=score.astype(np.float64))
    sums = sums[sums > 0]
    assert np.all(np.log2(sums) == np.rint(np.log2(sums))), "a user's ratings do not sum to a power of two"
    r = (0.5 * np.arange(1, 11)).astype(np.float32)
    for s in np.unique(sums).astype(np.float32):
        w = (r / s) / s                                               # the walk's weight of a rating, fp32
        assert np.array_equal(w.astype(np.float64), (r.astype(np.float64) / float(s)) / float(s))
        prod = w[:, None] * r[None, :]                                # fp32 products, either side: W_vi r_vj and W_vj r_vi
        exact = w.astype(np.float64)[:, None] * r.astype(np.float64)[None, :]
        assert prod.dtype == np.float32 and np.array_equal(prod.astype(np.float64), exact) and np.array_equal(prod, prod.T)
    env = {"FY_COOC_BLOCK": "256", "FY_COOC_MAX_CH": "768"}
    r0, s0, st0 = run("exact", {**env, "FY_COOC_RECT": "0"})
    r1, s1, st1 = run("exact", {**env, "FY_COOC_RECT": "1"})
    print({k: (st0[k], st1[k]) for k in STATS}, "segments", st0["cooc_segments"], st1["cooc_segments"])
    assert len(r1["user"]) > 0 and st1["blocks_total"] > 0
    assert st1["cooc_segments"] != st0["cooc_segments"], "both runs took the same walk"
    assert_same_bytes(r0, r1)
    assert_same_bytes(s0, s1)
    for k in STATS:
        assert st0[k] == st1[k], k
