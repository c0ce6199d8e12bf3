#!/usr/bin/env python3
"""Times requests for the similarity rows of named items (RowSimilarityJob.prepare + PreparedItemSimilarity.rows) beside the full build:
`python tools/itemsim_request_bench.py [--shape ml25m] [--measure SIMILARITY_COSINE,SIMILARITY_LOGLIKELIHOOD] [--sizes 1,100,10000]
 [--reps 5] [--k 100] [--out profiles/itemsim_request/ml25m.json] [--dump DIR]`.

The ratings are put into HBM once.  Per measure a job is prepared once and kept; after one warm-up of every configuration, `reps`
rounds ALTERNATE them in one run:
  full        RowSimilarityJob.run: the full build (fy_itemsim_build), whose code the request path does not touch
  rows:N      PreparedItemSimilarity.rows of N random items (fixed seed; the same items every round)
  rows:all    ... of every item
  prepare     RowSimilarityJob.prepare of a second job, closed again outside the timed window
`ms` is the HIP-event time of the whole call: two events recorded on the context's stream around the call, which ends
synchronised; `wall_ms` is the host clock around the same window.  Reported per configuration: median, minimum and spread
(max - min) over the rounds, and pair_contribs of a request.  The conditions of the request path, each against the full build OF
THE SAME RUN, are evaluated and printed, never enforced:
  rows:1 and rows:100 take less time than the full build (medians);
  prepare takes no longer than the full build plus the spread observed across the rounds (the larger of the two spreads).
`break_even_share`: the share of the items at which a request costs a full build, interpolated linearly between the two measured
request sizes that bracket the full build's median (None: every request, the all-items one included, is cheaper).  Nothing is
compared for correctness here: tests/test_itemsim_request_gpu.py does that.

`--dump DIR` writes the rows of the first request of each size (the items are fixed by --seed) as
DIR/<measure>.<rows:N>.{item,other,sim}.npy, in the order the request returned them, and DIR/stats.json with that request's recs and
request statistics: two builds of the library are compared byte for byte that way (`--reps 0` runs nothing else)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms, wall):
    return {"ms_runs": ms, "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_spread": float(max(ms) - min(ms)),
            "wall_ms_median": float(np.median(wall))}


def break_even(points, full_ms):
    """points: [(items, median ms)] ascending by items"""
    for (n0, t0), (n1, t1) in zip(points, points[1:]):
        if t0 <= full_ms < t1:
            return n0 + (n1 - n0) * (full_ms - t0) / (t1 - t0)
    return 0.0 if points[0][1] > full_ms else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--measure", default="SIMILARITY_COSINE,SIMILARITY_LOGLIKELIHOOD")
    ap.add_argument("--sizes", default="1,100,10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--seed", type=int, default=20261018)
    ap.add_argument("--out", default="")
    ap.add_argument("--dump", default="")
    a = ap.parse_args()
    dumped = {}
    import torch
    if not torch.cuda.is_available():
        sys.exit("itemsim_request_bench: no GPU (there is no CPU fallback and no CPU timing)")
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    user, item, score, facts = S.generate(a.shape, device=torch.device("cuda", 0))
    all_items = np.unique(item.cpu().numpy()).astype(np.int32)
    ctx = P.Context(0)
    R = P.Ratings(ctx, user, item, score)
    del user, item, score
    stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))
    rng = np.random.default_rng(a.seed)
    sizes = [min(int(x), len(all_items)) for x in a.sizes.split(",")]
    asked = {"rows:%d" % n: rng.choice(all_items, size=n, replace=False).astype(np.int32) for n in sizes}
    asked["rows:all"] = all_items
    configs = ["full"] + list(asked) + ["prepare"]
    out = {"shape": a.shape, "facts": {k: facts[k] for k in ("n_users", "n_items", "nnz")}, "reps": a.reps, "k": a.k, "measures": {}}

    for measure in a.measure.split(","):
        job = P.RowSimilarityJob(ctx)
        kw = dict(similarityClassname=measure, maxSimilaritiesPerRow=a.k)
        prepared = job.prepare(R, **kw)
        info = {}

        def run(name):
            ctx.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            if name == "full":
                res = job.run(R, **kw)
                info[name] = {"recs": res.stats["recs"], "pair_contribs": res.stats["pair_contribs"], "lib_ms_total": res.stats["ms_total"]}
            elif name == "prepare":
                res = job.prepare(R, **kw)
            else:
                res = prepared.rows(asked[name])
                info[name] = dict(res.request_stats, recs=res.stats["recs"], lib_ms_total=res.stats["ms_total"], lib_ms_cooc=res.stats["ms_cooc"],
                                  lib_ms_topn=res.stats["ms_topn"])
                if a.dump and (measure, name) not in dumped:
                    os.makedirs(a.dump, exist_ok=True)
                    for col, arr in res.rows().items():
                        np.save(os.path.join(a.dump, "%s.%s.%s.npy" % (measure, name.replace(":", "_"), col)), arr)
                    dumped[(measure, name)] = dict(res.request_stats, recs=res.stats["recs"], cooc_launches=res.stats["cooc_launches"])
                    with open(os.path.join(a.dump, "stats.json"), "w") as f:
                        json.dump({"%s.%s" % k: v for k, v in dumped.items()}, f, indent=1, sort_keys=True)
            e1.record(stream)
            e1.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            res.close()
            return e0.elapsed_time(e1), wall

        times = {c: ([], []) for c in configs}
        for c in configs:
            run(c)                                            # warm-up
        for _ in range(a.reps):
            for c in configs:
                ms, wall = run(c)
                times[c][0].append(ms)
                times[c][1].append(wall)
        prepared.close()
        if a.reps == 0:
            continue
        rec = {c: dict(summary(*times[c]), **info.get(c, {})) for c in configs}
        full = rec["full"]
        print("== %s, %s, K = %d, %d rounds" % (a.shape, measure, a.k, a.reps), flush=True)
        for c in configs:
            r = rec[c]
            print("%-12s %10.3f ms median  %10.3f min  (+- %.3f)  wall %10.3f  pair_contribs %s" % (
                c, r["ms_median"], r["ms_min"], r["ms_spread"], r["wall_ms_median"], r.get("pair_contribs", "-")), flush=True)
        spread = max(full["ms_spread"], rec["prepare"]["ms_spread"])
        cond = {name: bool(rec[name]["ms_median"] < full["ms_median"]) for name in asked if name != "rows:all" and int(name[5:]) <= 100}
        cond["prepare <= full + spread"] = bool(rec["prepare"]["ms_median"] <= full["ms_median"] + spread)
        points = [(len(asked[name]), rec[name]["ms_median"]) for name in asked]
        be = break_even(sorted(points), full["ms_median"])
        rec["conditions"] = cond
        rec["break_even_items"] = be
        rec["break_even_share"] = None if be is None else be / len(all_items)
        print("conditions:", cond, " break-even: %s items (%s of %d)" % (
            "none" if be is None else "%.0f" % be, "-" if be is None else "%.3f" % (be / len(all_items)), len(all_items)), flush=True)
        out["measures"][measure] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
