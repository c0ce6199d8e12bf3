#!/usr/bin/env python3
"""Times item-based lists for given profiles on a standing prepared job (PreparedItemSimilarity.recommend_profiles) beside what a
request right after a write costs without it:
`python tools/profile_bench.py [--shape ml25m] [--measure SIMILARITY_COSINE] [--sizes 1,100,10000] [--whole 1,1000] [--reps 5] [--k 100]
 [--n 100] [--max-prefs 50] [--out profiles/profiles/ml25m.json] [--dump DIR]`.

The ratings are put into HBM once and one job is prepared on them (the STANDING job).  Per request size n -- n random users with one
new rating each (score 5, an item the user has not rated) -- after one warm-up of every leg, `reps` rounds alternate the legs in one
run:
  A   today's route: Ratings.updated (the n writes) + prepare on the new ratings + recommend(users) on the new job's cold store
      (the three parts are also timed apart: A.update, A.prepare, A.recommend)
  B   recommend_profiles(base="resident") with the n writes on the standing job, its store dropped first (cold store)
  C   the same call again, on the warm store
  D   recommend(users) on the same warm store (run once untimed first, so that it builds nothing): the same pass without the ingest,
      so C - D is what the ingest costs
  E   (per --whole size m) m whole profiles of 20 preferences: E.cold on a dropped store, E.warm the same call again
`ms` is the HIP-event time of the whole call(s): two events recorded on the context's stream around them, every call ends
synchronised.  Reported per leg: median and min..max over the rounds, and the call's own statistics.  Note that A answers from
similarities that follow the write, B / C from the similarities as prepared: they are different answers by design
(include/filmyou.h).  Nothing is compared for correctness here: tests/test_profiles_gpu.py does that.
`--dump DIR`: the arrays and the integer statistics of the first result of every
leg as files (tools/_dump.py), to compare two builds of the library byte for byte."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _dump import Dump  # noqa: E402


def summary(ms):
    return {"ms_runs": ms, "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def new_ratings(h_user, h_item, users, all_items, rng):
    """one item per user that the user has not rated"""
    m = np.isin(h_user, users)
    have = set((h_user[m].astype(np.int64) << 32 | h_item[m].astype(np.int64)).tolist())
    items = rng.choice(all_items, size=len(users))
    for k, x in enumerate(users.tolist()):
        while (x << 32 | int(items[k])) in have:
            items[k] = rng.choice(all_items)
    return items.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--measure", default="SIMILARITY_COSINE")
    ap.add_argument("--sizes", default="1,100,10000")
    ap.add_argument("--whole", default="1,1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--max-prefs", type=int, default=50)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--out", default="")
    ap.add_argument("--dump", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("profile_bench: no GPU (there is no CPU fallback and no CPU timing)")
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    user, item, score, facts = S.generate(a.shape, device=torch.device("cuda", 0))
    h_user, h_item = user.cpu().numpy(), item.cpu().numpy()
    all_users, all_items = np.unique(h_user).astype(np.int32), np.unique(h_item).astype(np.int32)
    ctx = P.Context(0)
    R = P.Ratings(ctx, user, item, score)
    del user, item, score
    stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))
    rng = np.random.default_rng(a.seed)
    kw = dict(numRecommendations=a.n, maxPrefsPerUser=a.max_prefs)
    dump = Dump(a.dump)
    job = P.BaselineRecommenderJob(ctx)
    standing = job.prepare(R, maxSimilaritiesPerItem=a.k, similarityClassname=a.measure)
    out = {"shape": a.shape, "facts": {k: facts[k] for k in ("n_users", "n_items", "nnz")}, "measure": a.measure, "reps": a.reps, "k": a.k, "n": a.n,
           "max_prefs": a.max_prefs, "users": {}, "whole": {}}

    def timed(fn):
        ctx.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        res = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), res

    def note(info, leg, rec, stats):
        dump("%s.%s" % (dump_as, leg), rec, stats)
        info[leg] = dict(stats, recs=rec.stats["recs"], users_scored=rec.stats["users_scored"], lib_ms_tables=rec.stats["ms_tables"],
                         lib_ms_cooc=rec.stats["ms_cooc"], lib_ms_score=rec.stats["ms_score"], lib_ms_topn=rec.stats["ms_topn"])
        rec.close()

    def report(title, legs, times, info):
        rec = {leg: dict(summary(times[leg]), **info.get(leg, {})) for leg in legs}
        print("== " + title, flush=True)
        for leg in legs:
            r = rec[leg]
            print("%-12s %10.3f ms median  (%.3f .. %.3f)  built %s from store %s composed %s" % (
                leg, r["ms_median"], r["ms_min"], r["ms_max"], r.get("rows_built", "-"), r.get("rows_from_store", "-"), r.get("prefs_composed", "-")), flush=True)
        return rec

    for n in [min(int(x), len(all_users)) for x in a.sizes.split(",")]:
        users = rng.choice(all_users, size=n, replace=False).astype(np.int32)
        items = new_ratings(h_user, h_item, users, all_items, rng)
        scores = np.full(n, 5.0, dtype=np.float32)
        start = np.arange(n + 1, dtype=np.int64)
        profiles = (users, start, items, scores)
        info, dump_as = {}, "users_%d" % n

        def one_round():
            t = {}
            t["A.update"], R2 = timed(lambda: R.updated(users, items, scores))
            t["A.prepare"], fresh = timed(lambda: job.prepare(R2, maxSimilaritiesPerItem=a.k, similarityClassname=a.measure))
            t["A.recommend"], rec = timed(lambda: fresh.recommend(users, **kw))
            note(info, "A.recommend", rec, rec.request_stats)
            fresh.close()
            R2.close()
            t["A"] = t["A.update"] + t["A.prepare"] + t["A.recommend"]
            standing.drop_rows()
            for leg in ("B", "C"):
                t[leg], rec = timed(lambda: standing.recommend_profiles(profiles, base="resident", **kw))
                note(info, leg, rec, rec.profile_stats)
            standing.recommend(users, **kw).close()
            t["D"], rec = timed(lambda: standing.recommend(users, **kw))
            note(info, "D", rec, rec.request_stats)
            return t

        one_round()                                       # warm-up of every leg
        legs = ["A", "A.update", "A.prepare", "A.recommend", "B", "C", "D"]
        times = {leg: [] for leg in legs}
        for _ in range(a.reps):
            t = one_round()
            for leg in legs:
                times[leg].append(t[leg])
        rec = report("%s, %s, K = %d, N = %d, maxPrefs = %d, %d users with one new rating each, %d rounds" % (a.shape, a.measure, a.k, a.n, a.max_prefs, n, a.reps),
                     legs, times, info)
        rec["ingest_ms"] = rec["C"]["ms_median"] - rec["D"]["ms_median"]
        rec["B_over_A"] = rec["B"]["ms_median"] / rec["A"]["ms_median"]
        rec["C_over_A"] = rec["C"]["ms_median"] / rec["A"]["ms_median"]
        print("ingest (C - D) %.3f ms; B / A %.3f; C / A %.4f" % (rec["ingest_ms"], rec["B_over_A"], rec["C_over_A"]), flush=True)
        out["users"]["%d" % n] = rec

    for m in [int(x) for x in a.whole.split(",")]:
        start = np.arange(m + 1, dtype=np.int64) * 20
        items = np.concatenate([rng.choice(all_items, size=20, replace=False) for _ in range(m)]).astype(np.int32)
        scores = (rng.integers(1, 11, size=20 * m) / 2.0).astype(np.float32)
        profiles = (np.arange(m, dtype=np.int32) + int(all_users.max()) + 1, start, items, scores)
        info, dump_as = {}, "whole_%d" % m

        def whole_round():
            t = {}
            standing.drop_rows()
            for leg in ("E.cold", "E.warm"):
                t[leg], rec = timed(lambda: standing.recommend_profiles(profiles, base="whole", **kw))
                note(info, leg, rec, rec.profile_stats)
            return t

        whole_round()
        legs = ["E.cold", "E.warm"]
        times = {leg: [] for leg in legs}
        for _ in range(a.reps):
            t = whole_round()
            for leg in legs:
                times[leg].append(t[leg])
        out["whole"]["%d" % m] = report("%s, %s, %d whole profiles of 20 preferences, %d rounds" % (a.shape, a.measure, m, a.reps), legs, times, info)
    standing.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
