#!/usr/bin/env python3
"""Times the item-item similarity build for every measure: `python tools/itemsim_bench.py [--shape ml25m] [--k 100] [--reps 5]
[--out profiles/itemsim/measures_ml25m.json] [--job KEY=VALUE ...] [--dump DIR]`.

For each of the seven measures of include/filmyou.h at a `synth` shape: the build on the default route, with the symmetric
build forced where the measure admits it (FY_ISIM_GRAM=1) and on the forced row-at-a-time route (FY_ISIM_GRAM=0), one warm-up run
each, then `reps` timed runs, ALTERNATING the routes.  Reported per
(measure, route): every run's whole-build time (fy_stats ms_total: device time from the prepared structure to the compacted
rows) and its kernels' time (ms_cooc), the median and spread (max - min) of the whole build, unordered_pairs / s from the median,
and which route ran (symmetric = the upper triangle + band sweep, fy_stats isim_candidates > 0; otherwise row at a time).  The
ratings are resident (one Ratings object); nothing is compared here -- tests/test_itemsim_measures_gpu.py does that.

`--job KEY=VALUE` (repeatable; the value is JSON) passes a further argument to RowSimilarityJob.run: excludeSelfSimilarity=false,
threshold=0.25, world=2, rank=1, minPrefsPerUser=20, maxPrefsPerUser=100.  `--dump DIR` writes the rows of the first run of each
(measure, route) as DIR/<measure>.<route>.{item,other,sim}.npy, in the order the job returned them, and DIR/stats.json with that
run's recs, isim_candidates, isim_redone_rows and cooc_launches: two builds of the library are compared byte for byte that way
(`--reps 0` runs nothing else)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--measures", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--job", action="append", default=[], metavar="KEY=VALUE")
    ap.add_argument("--dump", default="")
    a = ap.parse_args()
    job_kw = {k: json.loads(v) for k, v in (kv.split("=", 1) for kv in a.job)}
    dumped = {}
    import torch
    if not torch.cuda.is_available():
        sys.exit("itemsim_bench: no GPU (there is no CPU fallback and no CPU timing)")
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    user, item, score, facts = S.generate(a.shape, device=torch.device("cuda", 0))
    ctx = P.Context(0)
    R = P.Ratings(ctx, user, item, score)
    job = P.RowSimilarityJob(ctx)
    measures = [m for m in a.measures.split(",") if m] or [P.SIMILARITY_COSINE, P.SIMILARITY_COOCCURRENCE, P.SIMILARITY_TANIMOTO_COEFFICIENT,
                                                            P.SIMILARITY_LOGLIKELIHOOD, P.SIMILARITY_CITY_BLOCK, P.SIMILARITY_EUCLIDEAN_DISTANCE,
                                                            P.SIMILARITY_PEARSON_CORRELATION]
    forced = os.environ.get("FY_ISIM_GRAM")
    ROUTES = ("default", "symmetric", "row_at_a_time")

    def run(measure, route):
        if route == "row_at_a_time":
            os.environ["FY_ISIM_GRAM"] = "0"
        elif route == "symmetric":
            os.environ["FY_ISIM_GRAM"] = "1"
        elif forced is None:
            os.environ.pop("FY_ISIM_GRAM", None)
        else:
            os.environ["FY_ISIM_GRAM"] = forced
        res = job.run(R, similarityClassname=measure, maxSimilaritiesPerRow=a.k, **job_kw)
        st = dict(res.stats)
        if a.dump and (measure, route) not in dumped:
            os.makedirs(a.dump, exist_ok=True)
            for name, arr in res.rows().items():
                np.save(os.path.join(a.dump, "%s.%s.%s.npy" % (measure, route, name)), arr)
            dumped[(measure, route)] = {k: st[k] for k in ("recs", "isim_candidates", "isim_redone_rows", "cooc_launches")}
            with open(os.path.join(a.dump, "stats.json"), "w") as f:
                json.dump({"%s.%s" % k: v for k, v in dumped.items()}, f, indent=1, sort_keys=True)
        res.close()
        return st

    out = {"shape": a.shape, "facts": {k: facts[k] for k in ("n_users", "n_items", "nnz")}, "k": a.k, "reps": a.reps, "measures": {}}
    for m in measures:
        rec = {}
        for route in ROUTES:
            run(m, route)                                     # warm-up
            rec[route] = {"ms_total_runs": [], "ms_cooc_runs": []}
        for _ in range(a.reps):
            for route in ROUTES:
                st = run(m, route)
                r = rec[route]
                r["ms_total_runs"].append(st["ms_total"])
                r["ms_cooc_runs"].append(st["ms_cooc"])
                r["route_ran"] = "symmetric" if st["isim_candidates"] > 0 else "row_at_a_time"
                r["unordered_pairs"] = st["unordered_pairs"]
                r["rows"] = st["recs"]
        if a.reps == 0:
            continue
        for r in rec.values():
            t = r["ms_total_runs"]
            r["ms_total_median"] = float(np.median(t))
            r["ms_total_spread"] = max(t) - min(t)
            r["ms_cooc_median"] = float(np.median(r["ms_cooc_runs"]))
            r["unordered_pairs_per_s"] = r["unordered_pairs"] / (1e-3 * r["ms_total_median"])
        out["measures"][m] = rec
        print("%-34s %s" % (m, " | ".join("%s: %s %.2f ms (+- %.2f) %.3e pairs/s" % (
            route, rec[route]["route_ran"], rec[route]["ms_total_median"], rec[route]["ms_total_spread"], rec[route]["unordered_pairs_per_s"])
            for route in ROUTES)), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
