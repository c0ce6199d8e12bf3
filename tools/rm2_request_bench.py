#!/usr/bin/env python3
"""Times RM2 requests of different sizes beside the warm full job: `python tools/rm2_request_bench.py [--shape ml25m]
[--clusters 1,50] [--n 50] [--sizes 1,100,10000] [--reps 5] [--out profiles/rm2_request/ml25m.json]`.

Per cluster count: the ratings are put into HBM once, one job is prepared (users hashed to equal clusters), the full job is run once
(warm-up: its tables are then cached on the job) and one request per size is run once (warm-up: the first request builds the job's
kept state).  Then `reps` rounds ALTERNATE the configurations in one run:
  full              PreparedRM2.score(): the warm full job
  users_<k>         PreparedRM2.score_users of k random users (fixed seed), the restricted pass forced (FY_REQ_FULL_SHARE=2)
Reported per configuration: every run's ms_total (HIP events on the context's stream around the whole call), its median and spread,
the per-phase medians (ms_tables: the request's plan; ms_cooc: slab build; ms_score; ms_topn), the request statistics, rows, and
`vs_full` = median over the median of `full`.  The switch point printed at the end is the share of a cluster's users at which the
restricted pass of an evenly spread request costs what the full job costs, interpolated between the measured sizes on a log scale
-- the basis of the default of fy::Tuning::req_full_share.  Nothing is compared here: tests/test_rm2_request_gpu.py does that."""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PHASES = ("ms_tables", "ms_cooc", "ms_score", "ms_topn")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--clusters", default="1,50")
    ap.add_argument("--n", type=int, default=50, help="numberOfRecommendations")
    ap.add_argument("--sizes", default="1,100,10000")
    ap.add_argument("--lam", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261018)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("rm2_request_bench: no GPU (there is no CPU fallback and no CPU timing)")
    os.environ["FY_REQ_FULL_SHARE"] = "2"
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    user, item, score, facts = S.generate(a.shape, device=torch.device("cuda", 0))
    all_users = torch.unique(user).cpu().numpy().astype(np.int32)
    ctx = P.Context(0)
    R = P.Ratings(ctx, user, item, score)
    del user, item, score
    sizes = [int(x) for x in a.sizes.split(",")]
    out = {"shape": a.shape, "facts": {k: facts[k] for k in ("n_users", "n_items", "nnz")}, "number_of_recommendations": a.n,
           "lambda": a.lam, "reps": a.reps, "runs": {}}
    for K in [int(x) for x in a.clusters.split(",")]:
        conf = P.Configuration()
        conf.set("lambda", repr(a.lam))
        conf.setInt("numberOfItems", facts["n_items"])
        conf.setInt("numberOfClusters", K)
        conf.setInt("numberOfRecommendations", a.n)
        job = P.RM2Job(conf, ctx).prepare(R, clustering=(all_users, S.hash_clustering(all_users, K)))
        rng = np.random.default_rng(a.seed)
        shuffled = rng.permutation(all_users)
        configs = {"full": None}
        for k in sizes:
            configs["users_%d" % k] = np.ascontiguousarray(shuffled[: min(k, len(shuffled))])

        def run(ids):
            rec = job.score() if ids is None else job.score_users(ids)
            st, rq = dict(rec.stats), rec.request_stats
            rec.close()
            return st, rq

        rec = {name: {"requested_users": None if ids is None else len(ids), "ms_total_runs": [], "phases": {p: [] for p in PHASES}}
               for name, ids in configs.items()}
        for ids in configs.values():
            run(ids)                                          # warm-up
        for _ in range(a.reps):
            for name, ids in configs.items():
                st, rq = run(ids)
                r = rec[name]
                r["ms_total_runs"].append(st["ms_total"])
                for p in PHASES:
                    r["phases"][p].append(st[p])
                r["users_scored"], r["rows"], r["request_stats"], r["pair_contribs"] = st["users_scored"], st["recs"], rq, st["pair_contribs"]
        full = float(np.median(rec["full"]["ms_total_runs"]))
        print("== %s, %d cluster(s), N = %d" % (a.shape, K, a.n), flush=True)
        for name, r in rec.items():
            t = r["ms_total_runs"]
            r["ms_total_median"] = float(np.median(t))
            r["ms_total_spread"] = max(t) - min(t)
            r["phases"] = {p + "_median": float(np.median(v)) for p, v in r["phases"].items()}
            r["vs_full"] = r["ms_total_median"] / full
            print("%-12s %10.3f ms (+- %.3f)  x%.3f of full  %7d users %9d rows  %s  %s" % (
                name, r["ms_total_median"], r["ms_total_spread"], r["vs_full"], r["users_scored"], r["rows"],
                " ".join("%s %.3f" % (k[3:-7], v) for k, v in r["phases"].items()), json.dumps(r["request_stats"])), flush=True)
        # share of a cluster's users at which the restricted pass costs the full job (log-log interpolation between the sizes)
        pts = [(r["requested_users"], r["ms_total_median"]) for n, r in rec.items() if n != "full"]
        switch = None
        for (k0, t0), (k1, t1) in zip(pts, pts[1:]):
            if t0 <= full < t1:
                kx = math.exp(math.log(k0) + (math.log(full) - math.log(t0)) * (math.log(k1) - math.log(k0)) / (math.log(t1) - math.log(t0)))
                switch = kx / len(all_users)
        if switch is None and pts:
            switch = 0.0 if pts[0][1] > full else pts[-1][0] / len(all_users)
        print("switch point (%d clusters): the restricted pass costs the full job at %.4f of the users (%s)" % (
            K, switch, "interpolated" if any(t0 <= full < t1 for (_, t0), (_, t1) in zip(pts, pts[1:])) else "outside the measured sizes"), flush=True)
        out["runs"][str(K)] = {"configs": rec, "switch_share": switch}
        job.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
