"""Ratings that are not fp16-exact through every flow a big cluster's RM2 job can take.

The job takes the packed row walk when every kept rating is exactly representable in fp16 and the unpacked walk otherwise
(fy_rm2_plan.hpp: use_pk; fy_cooc.hpp: cooc_accumulate_segments<false, double>, 8-byte CSR entries, ds_add_f64, the `else` branches of
cooc_rm2_epilogue_pack, refinement copies made from double accumulators).  One rating of 3.3 moves a whole job over.  The score patterns
of tests/rating_scales.py put the data sets of test_score_walk_gpu.py ("small") and test_cooc_epilogue_gpu.py ("wide") on both sides of
that gate; tests/test_rating_scales_cpu.py proves what this file takes for granted about them (which side, exact side outputs, exact
sums of "dyadic", |score| >= 1).  Oracle: oracle.rm2 with an unbounded list, compared by util.assert_topn_matches at util.RTOL, purely
relative.  ENV of test_cooc_epilogue_gpu.py forces the 24-bit format and the branch and bound at this size.

  (a) one cluster against the oracle: the default flow, fused bounds, the full pass, chunks of one and two blocks, two epilogue trips,
      lambda = 0; side outputs equal (tests/test_rating_scales_cpu.py: they are exact in fp64); 2^13 and 2^14 times the same integers,
      one on each side of the gate;
  (b) the variants of the unpacked walk agree byte for byte on "dyadic" -- both orientations, both epilogues, the lazy and the full
      mirror, both accumulator layouts, two runs, pruned and full pass.  The walk adds with fp64 atomics in an order that changes from
      run to run, so these identities hold ONLY because every sum of that data set is exact (no addition rounds): then the matrix is a
      pure function of the data, and a dropped, doubled or misplaced contribution, a block maximum too large or too small, or a copy
      read from the wrong place shows here as it does for the packed walk;
  (c) the refinement pass reading fp64 copies made from double accumulators;
  (d) FY_COOC_PK=0 on half stars: the same lists as the packed walk's within RTOL, side outputs equal;
  (e) six pruned clusters that stay dense on the lanes because the walk is unpacked (with half stars the same job takes panel mode),
      and twenty small clusters (the flat batch is the packed walk's: with tenths they run one after the other);
  (f) the cooperative path, one rank and two;
  (g) absolute discounting moves the walk: half stars minus 0.3 leave it, k + 2^-12 minus 2^-12 enters it; a Jelinek-Mercer job on
      the same ratings object afterwards is the job on a fresh object;
  (h) an update moves the walk and moves it back.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import rating_scales as RS
from test_cooc_epilogue_gpu import DATA, ENV, LAM, STATS, WIDE_ITEMS, assert_same_bytes, job, run
from test_pruned_coop_gpu import forced, run_threads, same_rows  # noqa: F401  (forced: a fixture)
from test_score_walk_gpu import N_ITEMS
from util import RTOL, assert_topn_matches, pkg

pytestmark = pytest.mark.gpu

for _name, _n in (("small", N_ITEMS), ("wide", WIDE_ITEMS)):
    for _pattern in ("tenths", "continuous", "one_inexact", "dyadic", "pow2_13", "pow2_14"):
        DATA["%s/%s" % (_pattern, _name)] = (functools.partial(RS.triples, _pattern, _name), _n)

BASE = {"small": {}, "wide": {"FY_COOC_BLOCK": "256"}}


@contextlib.contextmanager
def environment(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def copies(rec):
    return ({k: np.array(v, copy=True) for k, v in rec.rows().items()}, {k: np.array(v, copy=True) for k, v in rec.sums().items()},
            dict(rec.stats))


def conf_of(n_items, K, top_n, lam=LAM, smoothing=None, delta=None):
    conf = pkg().Configuration()
    if smoothing is None:
        conf.set("lambda", lam)
    else:
        conf.set("smoothing", smoothing)
        conf.set("delta", repr(float(delta)))
    conf.setInt("numberOfItems", n_items)
    conf.setInt("numberOfClusters", K)
    conf.setInt("numberOfRecommendations", top_n)
    return conf


@functools.lru_cache(maxsize=None)
def general_job(pattern, name, lam, K, top_n, env, base=True):
    """job() of test_cooc_epilogue_gpu.py with a lambda and a clustering: one job in a context of its own; cached."""
    P = pkg()
    with environment({**(ENV if base else {}), **dict(env)}):
        ctx = P.Context(0)
        rec = P.RM2Job(conf_of(RS.n_items_of(name), K, top_n, lam), ctx).run(RS.triples(pattern, name), clustering=RS.clustering(name, K))
        out = copies(rec)
        rec.close()
        ctx.close()
    return out


def check_sides(sums, st, ref):
    """user sums and the total are the oracle's numbers (exact in fp64 in any order), p(i|C) is one division away"""
    assert np.array_equal(sums["user_id"], ref["user_id"]) and np.array_equal(sums["item_id"], ref["item_id"])
    assert np.array_equal(sums["user_sum"], ref["user_sum"])
    assert sums["total_sum"] == ref["total_sum"]
    np.testing.assert_allclose(sums["item_coll"], ref["item_coll"], rtol=1e-15)
    assert st["log_terms"] == ref["log_terms"]


def assert_rows_close(a, b, rtol):
    """two jobs over the same problem: the same users with the same list lengths, the k-th score of every list within rtol (two scores
    closer than that may swap their items)"""
    assert np.array_equal(a["user"], b["user"]) and np.array_equal(a["cluster"], b["cluster"])
    x, y = a["score"].astype(np.float64), b["score"].astype(np.float64)
    fin = np.isfinite(y)
    assert np.array_equal(np.isfinite(x), fin) and np.array_equal(x[~fin], y[~fin])
    worst = float(np.max(np.abs(x[fin] - y[fin]) / np.abs(y[fin])))
    assert worst <= rtol, worst
    return worst


def pruned(st):
    assert st["blocks_total"] > 0, "the branch and bound did not run"
    assert st["blocks_survived"] > 0 and st["prune_fallbacks"] == 0


# ---------------------------------------------------------------- (a) against the oracle, one cluster
FLOWS = {"default": {}, "fused_bounds": {"FY_SUP_BOUNDS": "0"}, "full_pass": {"FY_PRUNE": "0"}, "chunks_256": {"FY_COOC_MAX_CH": "256"},
         "chunks_512": {"FY_COOC_MAX_CH": "512"}}


# A pruned batch whose survivors exceed a quarter of its blocks is redone by the full pass (FY_MAX_SURV_FRAC).  Where a pattern's bounds
# cannot bite, that knob is raised so that the survivor pass is what the test compares, as test_pruned_coop_gpu.py does:
#   * "continuous" on "small": ratings spread over 6000 : 1, so some item of every 256-column block rivals the seed's columns for every
#     rated item.  Measured at the default: 1798 of 1800 (user, block) pairs survive and the batch falls back (prune_fallbacks = 1); the
#     same bound in numpy fp64 with exact block maxima keeps 1799 of 1800 (339 for the half stars, 486 for tenths) -- it is the data;
#   * "dyadic" on "wide" (ratings spread over 4095 : 1): 1574 of 5400 survive, 29 %;
#   * "tenths" on "wide" in six clusters of 100 users: 4803 of 4993.
# With (almost) every block surviving, a block maximum that came out too small still drops a block somebody needs.
KEEP_SURVIVORS = {"FY_MAX_SURV_FRAC": "1e9"}


@pytest.mark.parametrize("flow", list(FLOWS))
@pytest.mark.parametrize("pattern", ["tenths", "continuous", "one_inexact"])
def test_one_cluster_against_the_oracle(pattern, flow):
    env = {**FLOWS[flow], **(KEEP_SURVIVORS if pattern == "continuous" and flow != "full_pass" else {})}
    rows, sums, st = run("%s/small" % pattern, env)
    ref = RS.reference(pattern, "small")
    worst = assert_topn_matches(rows, ref, 10)
    print("(a) %s small %s: worst relative error %.3g; blocks %d of %d, fallbacks %d, segments %d, select users %d"
          % (pattern, flow, worst, st["blocks_survived"], st["blocks_total"], st["prune_fallbacks"], st["cooc_segments"], st["topn_select_users"]))
    check_sides(sums, st, ref)
    if flow == "full_pass":
        assert st["blocks_total"] == 0
    else:
        pruned(st)


@pytest.mark.parametrize("max_ch", ["768", "1024"])
def test_two_epilogue_trips_against_the_oracle(max_ch):
    rows, sums, st = run("tenths/wide", {"FY_COOC_BLOCK": "256", "FY_COOC_MAX_CH": max_ch})
    ref = RS.reference("tenths", "wide")
    worst = assert_topn_matches(rows, ref, 10)
    print("(a) tenths wide chunks of %s: worst relative error %.3g; blocks %d of %d, segments %d" % (max_ch, worst, st["blocks_survived"], st["blocks_total"], st["cooc_segments"]))
    check_sides(sums, st, ref)
    pruned(st)


def test_lambda_zero():
    """a never co-rated pair is a zero term, the score -inf (quirk Q7): those rows stay; most seed lists end in -inf, no block can be
    excluded and the batch takes the full pass instead, as test_score_walk_gpu.py records for half stars"""
    rows, sums, st = general_job("tenths", "small", "0.0", 1, 10, ())
    ref = RS.reference("tenths", "small", "0.0")
    assert np.isneginf(ref["rec_score"]).any() and np.isneginf(rows["score"]).any()
    worst = assert_topn_matches(rows, ref, 10)
    print("(a) tenths small lambda = 0: worst relative error %.3g; blocks %d of %d, fallbacks %d" % (worst, st["blocks_survived"], st["blocks_total"], st["prune_fallbacks"]))
    check_sides(sums, st, ref)
    assert st["blocks_total"] > 0


def test_the_same_problem_on_both_sides_of_the_gate():
    """integers 1 ... 5 times 2^13 (40960 fits fp16: packed walk, magnitudes at the top of fp16) and times 2^14 (65536 overflows fp16:
    unpacked walk): the oracle's rows are the same floats (tests/test_rating_scales_cpu.py), so the two jobs answer one question"""
    r13, s13, st13 = run("pow2_13/small", {})
    r14, s14, st14 = run("pow2_14/small", {})
    ref13, ref14 = RS.reference("pow2_13", "small"), RS.reference("pow2_14", "small")
    w13 = assert_topn_matches(r13, ref13, 10)
    w14 = assert_topn_matches(r14, ref14, 10)
    check_sides(s13, st13, ref13)
    check_sides(s14, st14, ref14)
    pruned(st13)
    pruned(st14)
    between = assert_rows_close(r13, r14, RTOL)
    print("(a) pow2_13 (packed) / pow2_14 (unpacked): worst relative error %.3g / %.3g, between them %.3g; blocks %d of %d / %d of %d"
          % (w13, w14, between, st13["blocks_survived"], st13["blocks_total"], st14["blocks_survived"], st14["blocks_total"]))
    assert np.array_equal(s14["user_sum"], 2.0 * s13["user_sum"]) and np.array_equal(s14["item_coll"], s13["item_coll"])


# ---------------------------------------------------------------- (b) the variants of the unpacked walk, byte for byte
DYADIC = {"wide": {"FY_COOC_BLOCK": "256", "FY_COOC_MAX_CH": "768", **KEEP_SURVIVORS}, "small": {"FY_COOC_MAX_CH": "256"}}
VARIANTS = {"orientation": {"FY_COOC_RECT": "0"}, "epilogue": {"FY_COOC_EPI": "0"}, "mirror": {"FY_LAZY_MIRROR": "0"}, "layout": {"FY_COOC_PLANES": "0"},
            "again": None, "full_pass": {"FY_PRUNE": "0"}}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(DYADIC))
def test_unpacked_variants_agree_byte_for_byte(name, variant):
    """Every sum of "dyadic" is exact in fp64 (tests/test_rating_scales_cpu.py), so the order of the fp64 atomics does not show and
    the matrix, its block maxima and the refinement copies are pure functions of the data: any two ways of building them must agree
    in every byte of the rows, the side outputs and the five pruning statistics.  With data whose sums round, none of this holds."""
    data, env = "dyadic/%s" % name, DYADIC[name]
    r1, s1, st1 = run(data, env)
    pruned(st1)
    ref = RS.reference("dyadic", name)
    w1 = assert_topn_matches(r1, ref, 10)
    check_sides(s1, st1, ref)
    if VARIANTS[variant] is None:
        r0, s0, st0 = job.__wrapped__(data, 10, tuple(sorted(env.items())))          # past the cache: the job runs again
    else:
        r0, s0, st0 = run(data, {**env, **VARIANTS[variant]})
    w0 = assert_topn_matches(r0, ref, 10)
    print("(b) dyadic %s %s: worst relative error %.3g / %.3g; %s; segments %d / %d"
          % (name, variant, w1, w0, {k: (st1[k], st0[k]) for k in STATS}, st1["cooc_segments"], st0["cooc_segments"]))
    assert_same_bytes(r1, r0)
    assert_same_bytes(s1, s0)
    if variant == "full_pass":
        assert st0["blocks_total"] == 0
    else:
        for k in STATS:
            assert st1[k] == st0[k], k
    if variant == "orientation":
        assert st1["cooc_segments"] != st0["cooc_segments"], "both runs took the same walk"


# ---------------------------------------------------------------- (c) refinement from double accumulators
@pytest.mark.parametrize("max_ch", ["256", "512"])
def test_refinement_reads_copies_made_from_double_accumulators(max_ch):
    """test_cooc_rect_gpu.py: test_refinement_reads_the_tail_copies with tenths -- the fp64 copies (head32 / tail32) are the fp64
    accumulators of the unpacked epilogue times the scale in fp64 (MEpilogue::w2d); FY_REFINE_C raised until every list row whose item
    is a head column is scored again from them.  This test found the pass switched off for every job whose accumulators are not fixed
    point (rows_refined = 0: cluster_pass asked for fxk >= 0), i.e. for every job with one rating that is not fp16-exact; it now runs
    there too.  Measured: 89 897 rows re-scored, worst relative error 2.09e-7 with the pass, 2.79e-7 without."""
    env = {"FY_COOC_MAX_CH": max_ch, "FY_SEED_CHUNKS": "2", "FY_REFINE_C": "1000"}
    r0, s0, st0 = run("tenths/small", {**env, "FY_COOC_RECT": "0"}, 100)
    r1, s1, st1 = run("tenths/small", {**env, "FY_COOC_RECT": "1"}, 100)
    rn, sn, stn = run("tenths/small", {**env, "FY_COOC_RECT": "1", "FY_REFINE": "0"}, 100)
    assert st1["rows_refined"] > 0 and st1["rows_refined"] == st0["rows_refined"] and stn["rows_refined"] == 0
    assert st1["blocks_total"] > 0
    ref = RS.reference("tenths", "small")
    w0 = assert_topn_matches(r0, ref, 100)
    w1 = assert_topn_matches(r1, ref, 100)
    wn = assert_topn_matches(rn, ref, 100)
    print("(c) tenths small chunks of %s: rows refined %d / %d; worst relative error RECT=0 %.3g, RECT=1 %.3g, FY_REFINE=0 %.3g"
          % (max_ch, st0["rows_refined"], st1["rows_refined"], w0, w1, wn))
    assert w1 <= wn
    assert_same_bytes(s0, s1)
    check_sides(s1, st1, ref)


# ---------------------------------------------------------------- (d) the knob
@pytest.mark.parametrize("flow", ["default", "full_pass"])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_unpacked_walk_forced_onto_half_stars(name, flow):
    env = {**BASE[name], **FLOWS[flow]}
    rp, sp, stp = run(name, {**env, "FY_COOC_PK": "1"})
    ru, su, stu = run(name, {**env, "FY_COOC_PK": "0"})
    ref = RS.reference("half", name)
    wp = assert_topn_matches(rp, ref, 10)
    wu = assert_topn_matches(ru, ref, 10)
    between = assert_rows_close(ru, rp, RTOL)
    print("(d) half stars %s %s: worst relative error packed %.3g, FY_COOC_PK=0 %.3g, between them %.3g; blocks %d of %d / %d of %d"
          % (name, flow, wp, wu, between, stp["blocks_survived"], stp["blocks_total"], stu["blocks_survived"], stu["blocks_total"]))
    assert_same_bytes(sp, su)
    check_sides(su, stu, ref)
    if flow == "default":
        pruned(stu)
    else:
        assert stu["blocks_total"] == 0


# ---------------------------------------------------------------- (e) several clusters
def test_pruned_clusters_stay_dense_on_the_lanes():
    """Four or more pruned clusters take panel mode -- if the walk is packed (fy_rm2_plan.hpp).  Six clusters of tenths are pruned on
    dense matrices, one after the other on the lanes; the same job on half stars takes panel mode: the test stands on the gate."""
    env = (("FY_COOC_BLOCK", "256"),)
    rows, sums, st = general_job("tenths", "wide", LAM, 6, 10, env)
    ref = RS.reference("tenths", "wide", LAM, 6)
    worst = assert_topn_matches(rows, ref, 10)
    check_sides(sums, st, ref)
    rows_h, sums_h, st_h = general_job("half", "wide", LAM, 6, 10, env)
    worst_h = assert_topn_matches(rows_h, RS.reference("half", "wide", LAM, 6), 10)
    print("(e) wide in 6 clusters: tenths worst relative error %.3g, panel clusters %d, blocks %d of %d, fallbacks %d; half stars %.3g, panel clusters %d"
          % (worst, st["panel_clusters"], st["blocks_survived"], st["blocks_total"], st["prune_fallbacks"], worst_h, st_h["panel_clusters"]))
    assert st["panel_clusters"] == 0 and st["blocks_total"] > 0
    assert st_h["panel_clusters"] > 0
    # every cluster of that job fell back to the full pass (100 users: weak thresholds); with the fallback off the survivor pass of the
    # dense flow runs on every lane
    rows_s, sums_s, st_s = general_job("tenths", "wide", LAM, 6, 10, env + tuple(KEEP_SURVIVORS.items()))
    worst_s = assert_topn_matches(rows_s, ref, 10)
    print("(e) ... with the fallback off: worst relative error %.3g, blocks %d of %d, fallbacks %d" % (worst_s, st_s["blocks_survived"], st_s["blocks_total"], st_s["prune_fallbacks"]))
    assert st_s["panel_clusters"] == 0 and st_s["blocks_survived"] > 0 and st_s["prune_fallbacks"] == 0
    assert_same_bytes(sums, sums_s)


@pytest.mark.parametrize("env", [(), (("FY_M24_MIN_ITEMS", "64"),)], ids=["fp32_rows", "24_bit_rows"])
def test_many_small_clusters(env):
    """test_rm2_gpu.py: test_many_small_clusters_in_one_launch_per_kernel with tenths.  The flat batch needs the packed walk
    (fy_rm2_plan.hpp: `can`), so these twenty clusters run their chains one after the other: one scoring launch each."""
    rows, sums, st = general_job("tenths", "ml100k", LAM, 20, 30, env, False)
    ref = RS.reference("tenths", "ml100k", LAM, 20)
    worst = assert_topn_matches(rows, ref, 30)
    print("(e) tenths ml100k in 20 clusters %s: worst relative error %.3g, %d scoring launches" % (dict(env), worst, st["score_launches"]))
    check_sides(sums, st, ref)
    assert st["score_launches"] == 20


# ---------------------------------------------------------------- (f) the cooperative path
def test_cooperative_path(forced, monkeypatch):
    P = pkg()
    name, top_n = "ml100k", 20
    data, clustering, ref = RS.triples("tenths", name), RS.clustering(name, 1), RS.reference("tenths", name)
    conf = conf_of(RS.n_items_of(name), 1, top_n)
    monkeypatch.setenv("FY_COOP_FORCE", "1")
    ctx = P.Context(0)
    rec = P.RM2Job(conf, ctx).run(data, clustering=clustering)
    one, sums1, st1 = copies(rec)
    rec.close()
    ctx.close()
    assert st1["blocks_total"] > 0
    w1 = assert_topn_matches(one, ref, top_n)
    check_sides(sums1, st1, ref)
    monkeypatch.delenv("FY_COOP_FORCE")
    out, comms = run_threads(2, data, clustering, conf)
    two = {k: np.concatenate([o[0][k] for o in out]) for k in ("user", "item", "score", "cluster")}
    assert all(c.calls["reduce_scatter_f32"] >= 2 for c in comms), "the cluster was not scored cooperatively"
    w2 = assert_topn_matches(two, ref, top_n)
    print("(f) tenths ml100k cooperative: worst relative error one rank %.3g, two ranks %.3g; blocks %d of %d / %s of %s"
          % (w1, w2, st1["blocks_survived"], st1["blocks_total"], [o[1]["blocks_survived"] for o in out], [o[1]["blocks_total"] for o in out]))
    same_rows(two, one, tol=1e-6)       # what test_multirank_gpu.py grants exchanged partial sums of inexact scores


# ---------------------------------------------------------------- (g) discounting moves the walk
@pytest.mark.parametrize("flow", ["default", "full_pass"])
@pytest.mark.parametrize("pattern,delta", [("half", RS.DELTA_OUT), ("plus_2^-12", RS.DELTA_IN)], ids=["leaves_the_packed_walk", "enters_the_packed_walk"])
def test_discounting_moves_the_walk(pattern, delta, flow):
    """k_discount_not_fp16 judges r' = r - delta again.  Half stars minus 0.3: packed prep, then the unpacked walk.  k + 2^-12 minus
    2^-12: r' is an integer and the walk is packed while the ratings object says "not fp16-exact".  Then a Jelinek-Mercer job on the
    SAME ratings object (another cache key): it walks r, not r', and is the job on a fresh object bit for bit."""
    P = pkg()
    data, clustering = RS.triples(pattern, "small"), RS.clustering("small", 1)
    with environment({**ENV, **FLOWS[flow]}):
        ctx = P.Context(0)
        kept = P.Ratings(ctx, *data)
        rec = P.RM2Job(conf_of(N_ITEMS, 1, 10, smoothing="absoluteDiscounting", delta=delta), ctx).run(kept, clustering=clustering)
        rows, sums, st = copies(rec)
        rec.close()
        jm = P.RM2Job(conf_of(N_ITEMS, 1, 10), ctx)
        rec = jm.run(kept, clustering=clustering)
        rows_jm, sums_jm, st_jm = copies(rec)
        rec.close()
        fresh = P.Ratings(ctx, *data)
        rec = jm.run(fresh, clustering=clustering)
        rows_fresh, sums_fresh, st_fresh = copies(rec)
        rec.close()
        fresh.close()
        kept.close()
        ctx.close()
    worst = assert_topn_matches(rows, RS.smoothing_reference(pattern, "small", "absoluteDiscounting", delta), 10)
    ref = RS.reference(pattern, "small")
    worst_jm = assert_topn_matches(rows_jm, ref, 10)
    print("(g) %s minus %g, %s: worst relative error %.3g, blocks %d of %d; Jelinek-Mercer afterwards %.3g, blocks %d of %d"
          % (pattern, delta, flow, worst, st["blocks_survived"], st["blocks_total"], worst_jm, st_jm["blocks_survived"], st_jm["blocks_total"]))
    assert (st["blocks_total"] > 0) == (flow == "default")
    assert st_fresh["prepared_from_cache"] == 0
    check_sides(sums_jm, st_jm, ref)
    # (half stars: the packed walk, bit-reproducible.  k + 2^-12: the unpacked walk, whose fp64 sums may differ in their last bit with the
    # order of the atomics -- a row shows that only where 2^-53 crosses a rounding boundary of the fp32 element or score)
    assert_same_bytes(rows_jm, rows_fresh)
    assert_same_bytes(sums_jm, sums_fresh)
    assert_same_bytes({k: sums[k] for k in ("user_id", "user_sum", "item_id")}, {k: sums_jm[k] for k in ("user_id", "user_sum", "item_id")})


# ---------------------------------------------------------------- (h) an update moves the walk
def test_an_update_moves_the_walk_and_back():
    """fy_ratings_apply judges exactness again after a batch.  Half stars (packed) -> one rating upserted to 3.3 (unpacked: the
    oracle's rows of the updated data) -> upserted back, or deleted (packed again: the packed walk is bit-reproducible, so the rows are
    those of the job before the update, or of a fresh object without that rating, in every byte)."""
    from test_rm2_request_gpu import check, expected
    P = pkg()
    user, item, score = RS.triples("half", "small")
    at = RS.the_inexact_entry("small")
    key = (user[at:at + 1].copy(), item[at:at + 1].copy())
    clustering = RS.clustering("small", 1)

    def run_on(job_, ratings):
        rec = job_.run(ratings, clustering=clustering)
        out = copies(rec)
        rec.close()
        return out
    with environment(ENV):
        ctx = P.Context(0)
        rm2 = P.RM2Job(conf_of(N_ITEMS, 1, 10), ctx)
        R = P.Ratings(ctx, user, item, score)
        a_rows, a_sums, a_st = run_on(rm2, R)
        U = R.updated(key[0], key[1], np.array([RS.INEXACT], dtype=np.float32))
        assert U.update_stats["n_replaced"] == 1 and U.update_stats["nnz_out"] == len(user)
        b_rows, b_sums, b_st = run_on(rm2, U)
        back = U.updated(key[0], key[1], score[at:at + 1])
        c_rows, c_sums, c_st = run_on(rm2, back)
        gone = U.updated(key[0], key[1], np.zeros(1, dtype=np.float32), np.ones(1, dtype=np.uint8))
        assert gone.update_stats["n_deleted"] == 1 and gone.update_stats["nnz_out"] == len(user) - 1
        d_rows, d_sums, d_st = run_on(rm2, gone)
        direct = P.Ratings(ctx, *RS.triples("one_removed", "small"))
        e_rows, e_sums, e_st = run_on(rm2, direct)
        # on request, from the updated, inexact object
        ref_b = RS.reference("one_inexact", "small")
        asked = np.unique(np.concatenate([key[0], np.unique(user)[[0, 11, 450, 898]]])).astype(np.int32)
        prepared = rm2.prepare(U, clustering=clustering)
        try:
            req = prepared.score_users(asked)
            w_req = check(req, expected(ref_b, asked), 10)
            req.close()
        finally:
            prepared.close()
        for x in (direct, gone, back, U, R):
            x.close()
        ctx.close()
    w_a = assert_topn_matches(a_rows, RS.reference("half", "small"), 10)
    w_b = assert_topn_matches(b_rows, ref_b, 10)
    check_sides(b_sums, b_st, ref_b)
    ref_d = RS.reference("one_removed", "small")
    w_d = assert_topn_matches(d_rows, ref_d, 10)
    check_sides(d_sums, d_st, ref_d)
    print("(h) worst relative error: before %.3g, with 3.3 %.3g, without the rating %.3g, request %.3g; blocks %d of %d / %d of %d / %d of %d"
          % (w_a, w_b, w_d, w_req, a_st["blocks_survived"], a_st["blocks_total"], b_st["blocks_survived"], b_st["blocks_total"], d_st["blocks_survived"], d_st["blocks_total"]))
    assert not np.array_equal(a_rows["score"], b_rows["score"])       # the update shows
    assert_same_bytes(a_rows, c_rows)
    assert_same_bytes(a_sums, c_sums)
    for k in STATS:
        assert a_st[k] == c_st[k], k
    assert_same_bytes(d_rows, e_rows)
    assert_same_bytes(d_sums, e_sums)
    for k in STATS:
        assert d_st[k] == e_st[k], k
