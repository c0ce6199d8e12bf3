#!/usr/bin/env python3
"""Times explanations of named pairs (PreparedItemSimilarity.because) beside the estimates of the same pairs
(PreparedItemSimilarity.estimate) on the same warm row store:
`python tools/because_bench.py [--shape ml25m] [--measure SIMILARITY_COSINE] [--fraction 0.1] [--reps 5] [--k 100] [--max-prefs 50]
 [--how-many 5] [--out profiles/because/ml25m.json] [--dump DIR]`.

The ratings are generated in HBM and split once (Ratings.holdout(fraction, seed 1)); ONE job is prepared on the train side.  Three
requests, their pairs resident in HBM:
  web     one user x the 50 items of its list (recommend, N = 50)
  users   1000 users x the 20 items of their lists
  test    the pairs of the test side
Each request is first answered once by both calls (the rows it needs are then in the store, both kernels have run), then `reps`
rounds alternate because / estimate.  Reported per request and call: median and min .. max over the rounds of the library's own
HIP-event times (ms_total, ms_tables, ms_score), the because / estimate ratio of the ms_total and ms_score medians, and
row_entries_walked of both.  Nothing is compared for correctness here: tests/test_because_gpu.py does that.
`--dump DIR`: the arrays and the integer statistics of the first result of every
request and call as files (tools/_dump.py), to compare two builds of the library byte for byte."""
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
    return {"runs": ms, "median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--measure", default="SIMILARITY_COSINE")
    ap.add_argument("--fraction", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--max-prefs", type=int, default=50)
    ap.add_argument("--how-many", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--dump", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("because_bench: no GPU (there is no CPU fallback and no CPU timing)")
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    dev = torch.device("cuda", 0)
    user, item, score, facts = S.generate(a.shape, device=dev)
    ctx = P.Context(0)
    R = P.Ratings(ctx, user, item, score)
    del user, item, score
    train, test = R.holdout(a.fraction, seed=1)
    R.close()
    tu, ti, _ = test.to_host()
    test_users = np.unique(tu).astype(np.int32)
    dump = Dump(a.dump)
    prepared = P.BaselineRecommenderJob(ctx).prepare(train, maxSimilaritiesPerItem=a.k, similarityClassname=a.measure)

    def list_pairs(users, n):
        rows = prepared.recommend(users, numRecommendations=n, maxPrefsPerUser=a.max_prefs).rows()
        return rows["user"].astype(np.int32), rows["item"].astype(np.int32)

    some = test_users[:: max(1, len(test_users) // 1000)][:1000]
    requests = {}
    for k in range(len(some)):                                  # the first of them with a full list
        pu, pi = list_pairs(some[k:k + 1], 50)
        if len(pu) == 50:
            requests["web"] = (pu, pi)
            break
    requests["users"] = list_pairs(some, 20)
    requests["test"] = (tu.astype(np.int32), ti.astype(np.int32))
    out = {"shape": a.shape, "facts": {k: facts[k] for k in ("n_users", "n_items", "nnz")}, "measure": a.measure, "fraction": a.fraction,
           "reps": a.reps, "k": a.k, "max_prefs": a.max_prefs, "how_many": a.how_many, "train": train.nnz, "test": test.nnz, "requests": {}}
    print("== %s, %s, K = %d, maxPrefs = %d, howMany = %d, holdout %.2f: %d train, %d test pairs, %d rounds" % (
        a.shape, a.measure, a.k, a.max_prefs, a.how_many, a.fraction, train.nnz, test.nnz, a.reps), flush=True)
    for name, (pu, pi) in requests.items():
        pairs = (torch.from_numpy(pu).to(dev), torch.from_numpy(pi).to(dev))
        calls = {"because": lambda: prepared.because(pairs, howMany=a.how_many, maxPrefsPerUser=a.max_prefs),
                 "estimate": lambda: prepared.estimate(pairs, maxPrefsPerUser=a.max_prefs)}
        series, info = {}, {}
        for keep in [False] + [True] * a.reps:                  # one round to fill the store and warm both kernels, then the rounds that count
            for call, fn in calls.items():
                res = fn()
                dump("%s.%s" % (name, call), res, res.because_stats if call == "because" else res.estimate_stats)
                if keep:
                    for k in ("ms_total", "ms_tables", "ms_score"):
                        series.setdefault("%s.%s" % (call, k), []).append(float(res.stats[k]))
                    st = res.because_stats if call == "because" else res.estimate_stats
                    assert st["rows_built"] == 0
                    info[call] = {k: st[k] for k in ("pairs_asked", "targets", "users_known", "by_status", "row_entries_walked")}
                    if call == "because":
                        info[call].update(rows=st["rows"], contributors=st["contributors"])
                res.close()
        ms = {k: summary(v) for k, v in series.items()}
        ratio = {k: ms["because." + k]["median"] / ms["estimate." + k]["median"] for k in ("ms_total", "ms_score")}
        out["requests"][name] = {"pairs": len(pu), "ms": ms, "because/estimate": ratio, **info}
        print("-- %s: %d pairs" % (name, len(pu)), flush=True)
        for k, v in ms.items():
            print("%-22s %12.3f median  (%.3f .. %.3f)" % (k, v["median"], v["min"], v["max"]), flush=True)
        print("because / estimate: ms_total %.2f, ms_score %.2f; row_entries_walked %d / %d" % (
            ratio["ms_total"], ratio["ms_score"], info["because"]["row_entries_walked"], info["estimate"]["row_entries_walked"]), flush=True)
        print("because:", info["because"], flush=True)
    prepared.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
