#!/usr/bin/env python3
"""Times estimated preferences for the pairs of a hold-out (PreparedItemSimilarity.estimate + PreferenceEstimates.errors) beside the
list pass of the same users on the same job:
`python tools/estimate_bench.py [--shape ml25m] [--measure SIMILARITY_COSINE] [--fraction 0.1] [--reps 5] [--k 100] [--n 10]
 [--max-prefs 50] [--out profiles/estimate/ml25m.json] [--dump DIR]`.

The ratings are generated in HBM and split once (Ratings.holdout(fraction, seed 1)).  After one warm-up of every leg, `reps` rounds
run the legs in one process, each round on a NEW prepared job of the train side:
  cold       estimate(test) on the cold row store: every row the test users' kept preferences need is built
  warm       the same call again, on the store `cold` left
  errors     errors(test) of the warm result (the call's own HIP-event time, `ms` of fy_eval_errors)
  recommend  recommend(users of the test side, numRecommendations = n) on the same warm store: the list pass of the same users
Reported per leg: median and spread (max - min) over the rounds of the library's own HIP-event times (ms_total, ms_score, and for the
list pass ms_score + ms_topn), pairs per second of the warm estimate, its statistics (row_entries_walked among them) and MAE / RMSE.
The expectation -- the warm estimate's ms_score does not exceed the list pass's ms_score + ms_topn by more than the larger spread --
is evaluated and printed, never enforced.  Nothing is compared for correctness here: tests/test_estimate_gpu.py does that.
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
    return {"runs": ms, "median": float(np.median(ms)), "min": float(min(ms)), "spread": float(max(ms) - min(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--measure", default="SIMILARITY_COSINE")
    ap.add_argument("--fraction", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--max-prefs", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--dump", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("estimate_bench: no GPU (there is no CPU fallback and no CPU timing)")
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    user, item, score, facts = S.generate(a.shape, device=torch.device("cuda", 0))
    ctx = P.Context(0)
    R = P.Ratings(ctx, user, item, score)
    del user, item, score
    train, test = R.holdout(a.fraction, seed=1)
    R.close()
    test_users = np.unique(test.to_host()[0]).astype(np.int32)
    job = P.BaselineRecommenderJob(ctx)
    out = {"shape": a.shape, "facts": {k: facts[k] for k in ("n_users", "n_items", "nnz")}, "measure": a.measure, "fraction": a.fraction,
           "reps": a.reps, "k": a.k, "n": a.n, "max_prefs": a.max_prefs, "train": train.nnz, "test": test.nnz, "test_users": len(test_users)}
    series = {}
    info = {}
    dump = Dump(a.dump)

    def note(name, value):
        series.setdefault(name, []).append(float(value))

    def one_round(keep):
        prepared = job.prepare(train, maxSimilaritiesPerItem=a.k, similarityClassname=a.measure)
        cold = prepared.estimate(test, maxPrefsPerUser=a.max_prefs)
        warm = prepared.estimate(test, maxPrefsPerUser=a.max_prefs)
        err = warm.errors(test)
        rec = prepared.recommend(test_users, numRecommendations=a.n, maxPrefsPerUser=a.max_prefs)
        dump("cold", cold, cold.estimate_stats)
        dump("warm", warm, warm.estimate_stats)
        dump("recommend", rec, rec.request_stats)
        if keep:
            for leg, res in (("cold", cold), ("warm", warm)):
                for k in ("ms_total", "ms_tables", "ms_cooc", "ms_score"):
                    note("%s.%s" % (leg, k), res.stats[k])
            note("warm.pairs_per_s", warm.size / (warm.stats["ms_total"] * 1e-3))
            note("errors.ms", err.ms)
            for k in ("ms_total", "ms_tables", "ms_score", "ms_topn"):
                note("recommend.%s" % k, rec.stats[k])
            note("recommend.ms_score+ms_topn", rec.stats["ms_score"] + rec.stats["ms_topn"])
            info["cold"], info["warm"] = cold.estimate_stats, warm.estimate_stats
            info["errors"] = {"pairs": err.pairs, "estimated": err.estimated, "by_status": err.by_status, "mae": err.mae, "rmse": err.rmse,
                              "bias": err.bias, "coverage": err.coverage}
            info["recommend"] = dict(rec.request_stats, recs=rec.stats["recs"], users_scored=rec.stats["users_scored"])
        for x in (cold, warm, rec, prepared):
            x.close()

    one_round(False)                                          # warm-up of every leg
    for _ in range(a.reps):
        one_round(True)
    out["ms"] = {k: summary(v) for k, v in series.items()}
    out.update(info)
    est, lst = out["ms"]["warm.ms_score"], out["ms"]["recommend.ms_score+ms_topn"]
    out["warm ms_score <= list ms_score + ms_topn (within the spread)"] = bool(est["median"] - lst["median"] <= max(est["spread"], lst["spread"]))
    print("== %s, %s, K = %d, maxPrefs = %d, holdout %.2f: %d train, %d test pairs of %d users, %d rounds" % (
        a.shape, a.measure, a.k, a.max_prefs, a.fraction, train.nnz, test.nnz, len(test_users), a.reps), flush=True)
    for k, v in out["ms"].items():
        print("%-28s %14.3f median  (+- %.3f)" % (k, v["median"], v["spread"]), flush=True)
    print("warm estimate:", info["warm"], flush=True)
    print("errors:", info["errors"], flush=True)
    print("recommend (N = %d):" % a.n, info["recommend"], flush=True)
    print("warm ms_score <= list ms_score + ms_topn (within the spread):", out["warm ms_score <= list ms_score + ms_topn (within the spread)"], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
