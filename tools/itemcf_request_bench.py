#!/usr/bin/env python3
"""Times item-based recommendations for named users from a prepared similarity job (BaselineRecommenderJob.prepare +
PreparedItemSimilarity.recommend) beside what such a request costs after a write without it:
`python tools/itemcf_request_bench.py [--shape ml25m] [--measure SIMILARITY_COSINE,SIMILARITY_LOGLIKELIHOOD] [--sizes 1,100,10000]
 [--reps 5] [--k 100] [--n 100] [--max-prefs 50] [--out profiles/itemcf_request/ml25m.json] [--dump DIR]`.

The ratings are put into HBM once.  Per measure and request size, after one warm-up of every leg, `reps` rounds ALTERNATE the legs
in one run:
  A   RowSimilarityJob.run (the whole matrix), then BaselineRecommenderJob.run(similarities=, usersFile=): today's request after a write
  B   prepare + recommend on the cold store of the new job (the two parts are also timed apart: B.prepare, B.recommend)
  C   the same request again, on the store B left
  D   a different request of the same size on the store C left, with the share of its rows that came from the store
`ms` is the HIP-event time of the whole call(s): two events recorded on the context's stream around them, every call ends
synchronised.  Reported per leg: median and spread (max - min) over the rounds, the request statistics, and the walk of the
heaviest row B had to build (sum over the raters of the row's item of their number of preferences -- one workgroup per column
chunk walks all of it).  The conditions, each against other legs OF THE SAME RUN and only where the difference exceeds the larger
of the two spreads, are evaluated and printed, never enforced:
  B < A for the 1-user request with SIMILARITY_LOGLIKELIHOOD;
  C < B.recommend for both measures at every size.
Nothing is compared for correctness here: tests/test_itemcf_request_gpu.py does that.
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
    return {"ms_runs": ms, "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_spread": float(max(ms) - min(ms))}


def less(a, b):
    """a's median is below b's by more than the larger spread"""
    return bool(b["ms_median"] - a["ms_median"] > max(a["ms_spread"], b["ms_spread"]))


def heaviest_built_row(user, item, score, walk, users, max_prefs):
    """-> (item id, walk) of the heaviest item among the kept preferences of the requested users (numpy, host)"""
    m = np.isin(user, users)
    u, i, s = user[m], item[m], score[m]
    order = np.lexsort((-s, u))
    u, i, s = u[order], i[order], s[order]
    first = np.r_[0, np.flatnonzero(u[1:] != u[:-1]) + 1]
    length = np.diff(np.r_[first, len(u)])
    cut = first + np.minimum(length, max_prefs) - 1
    thr = np.repeat(s[cut], length)
    kept = np.unique(i[s >= thr])
    top = kept[np.argmax(walk[kept])]
    return int(top), int(walk[top])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--measure", default="SIMILARITY_COSINE,SIMILARITY_LOGLIKELIHOOD")
    ap.add_argument("--sizes", default="1,100,10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--max-prefs", type=int, default=50)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--out", default="")
    ap.add_argument("--dump", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("itemcf_request_bench: no GPU (there is no CPU fallback and no CPU timing)")
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    user, item, score, facts = S.generate(a.shape, device=torch.device("cuda", 0))
    h_user, h_item, h_score = user.cpu().numpy(), item.cpu().numpy(), score.cpu().numpy()
    all_users = np.unique(h_user).astype(np.int32)
    deg = np.bincount(h_user)
    walk = np.bincount(h_item, weights=deg[h_user].astype(np.float64)).astype(np.int64)
    ctx = P.Context(0)
    R = P.Ratings(ctx, user, item, score)
    del user, item, score
    stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))
    rng = np.random.default_rng(a.seed)
    sizes = [min(int(x), len(all_users) // 2) for x in a.sizes.split(",")]
    kw = dict(numRecommendations=a.n, maxPrefsPerUser=a.max_prefs)
    dump = Dump(a.dump)
    out = {"shape": a.shape, "facts": {k: facts[k] for k in ("n_users", "n_items", "nnz")}, "reps": a.reps, "k": a.k, "n": a.n,
           "max_prefs": a.max_prefs, "measures": {}}

    def timed(fn):
        ctx.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        res = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), res

    for measure in a.measure.split(","):
        job, sim_job = P.BaselineRecommenderJob(ctx), P.RowSimilarityJob(ctx)
        out["measures"][measure] = {}
        for n in sizes:
            both = rng.choice(all_users, size=2 * n, replace=False).astype(np.int32)
            first, other = both[:n], both[n:]
            info = {}

            def leg_a():
                sims = sim_job.run(R, measure, a.k, True, None)
                rec = job.run(R, similarities=sims, usersFile=first, **kw)[0]
                info["A"] = {"recs": rec.stats["recs"], "users_scored": rec.stats["users_scored"]}
                rec.close()
                sims.close()

            def one_round():
                t = {}
                t["A"], _ = timed(leg_a)
                t["B.prepare"], prepared = timed(lambda: job.prepare(R, maxSimilaritiesPerItem=a.k, similarityClassname=measure))
                for leg, users in (("B.recommend", first), ("C", first), ("D", other)):
                    t[leg], rec = timed(lambda: prepared.recommend(users, **kw))
                    dump("%s.users_%d.%s" % (measure, n, leg), rec, rec.request_stats)
                    info[leg] = dict(rec.request_stats, recs=rec.stats["recs"], users_scored=rec.stats["users_scored"],
                                     lib_ms_tables=rec.stats["ms_tables"], lib_ms_cooc=rec.stats["ms_cooc"], lib_ms_score=rec.stats["ms_score"],
                                     lib_ms_topn=rec.stats["ms_topn"], lib_ms_total=rec.stats["ms_total"])
                    rec.close()
                prepared.close()
                t["B"] = t["B.prepare"] + t["B.recommend"]
                return t

            one_round()                                       # warm-up of every leg
            legs = ["A", "B", "B.prepare", "B.recommend", "C", "D"]
            times = {leg: [] for leg in legs}
            for _ in range(a.reps):
                t = one_round()
                for leg in legs:
                    times[leg].append(t[leg])
            rec = {leg: dict(summary(times[leg]), **info.get(leg, {})) for leg in legs}
            d = info["D"]
            rec["D"]["from_store_share"] = d["rows_from_store"] / max(1, d["items_needed"])
            heavy_item, heavy_walk = heaviest_built_row(h_user, h_item, h_score, walk, first, a.max_prefs)
            rec["heaviest_built_row"] = {"item": heavy_item, "walk": heavy_walk}
            cond = {"C < B.recommend": less(rec["C"], rec["B.recommend"])}
            if n == 1:
                cond["B < A"] = less(rec["B"], rec["A"])
            rec["conditions"] = cond
            print("== %s, %s, K = %d, N = %d, maxPrefs = %d, %d users, %d rounds" % (a.shape, measure, a.k, a.n, a.max_prefs, n, a.reps), flush=True)
            for leg in legs:
                r = rec[leg]
                print("%-12s %10.3f ms median  (+- %.3f)  built %s from store %s pair_contribs %s" % (
                    leg, r["ms_median"], r["ms_spread"], r.get("rows_built", "-"), r.get("rows_from_store", "-"), r.get("pair_contribs", "-")), flush=True)
            print("heaviest built row: item %d, walk %d; D from the store: %.3f; conditions: %s" % (
                heavy_item, heavy_walk, rec["D"]["from_store_share"], cond), flush=True)
            out["measures"][measure]["users:%d" % n] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
