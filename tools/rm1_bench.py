"""The RM1 estimator next to RM2 ("RM1 estimator").

    python tools/rm1_bench.py [--jobs ml1m:1 ml1m:50 ml25m:50] [--requests 1 100 10000] [--request-shape ml25m:50] [--reps 3]
                              [--top-n 50] [--out profiles/rm1/<name>.json]

Per (shape, numberOfClusters) of --jobs: one resident ratings object, Jelinek-Mercer lambda 0.1; after one warm-up job of each
estimator, `reps` warm jobs (the kept state of the ratings object serves both estimators) of RM2 and of RM1.  Then, on
--request-shape, one fy_rm2_score_users call of an RM1 job per size of --requests (the first n users of a fixed permutation), `reps`
times each.  Times are HIP-event milliseconds on the context's stream; a job's time is ms_prepare + ms_total of fy_stats.  Printed
per line, and as one JSON document: the median job time of both estimators and their ratio, and for RM1 the two work counts of
DESIGN.md section 2g (pair_contribs = entries of the neighbours' rows tested, log_terms = column entries gathered), the seconds per
phase (tables, likelihoods + weights, scores, top-N) and the entries per second of each product.

One cluster of the whole ML-25M shape (--jobs ml25m:1) is 162 541 x 25 M = 4e12 entries per product; it is not in the default
list, and BASELINE.md says what it costs."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("ms_prepare", "ms_tables", "ms_cooc", "ms_score", "ms_topn", "ms_total")


def conf_of(P, model, n_items, K, top_n):
    conf = P.Configuration()
    conf.set("relevanceModel", model)
    conf.set("lambda", "0.1")
    conf.setInt("numberOfItems", n_items)
    conf.setInt("numberOfClusters", K)
    conf.setInt("numberOfRecommendations", top_n)
    return conf


def summary(sts):
    t = np.array([x["ms_prepare"] + x["ms_total"] for x in sts])
    out = {"ms_job_median": float(np.median(t)), "ms_job_min": float(t.min()), "ms_job_max": float(t.max())}
    out.update({k: float(np.median([x[k] for x in sts])) for k in PHASES})
    for k in ("pair_contribs", "log_terms", "users_scored", "recs", "cooc_launches"):
        out[k] = int(sts[-1][k])
    return out


def rates(r):
    r["loglik_entries_per_s"] = r["pair_contribs"] / (r["ms_cooc"] * 1e-3) if r["ms_cooc"] > 0 else None
    r["gather_entries_per_s"] = r["log_terms"] / (r["ms_score"] * 1e-3) if r["ms_score"] > 0 else None
    return r


def load(P, S, ctx, shape, K):
    import torch
    user, item, score, facts = S.generate(shape, device=torch.device("cuda", 0))
    ratings = P.Ratings(ctx, user, item, score)
    clustering = None
    if K > 1:
        uu = np.arange(1, facts["n_users"] + 1, dtype=np.int32)
        clustering = (uu, S.hash_clustering(uu, K))
    return ratings, clustering, facts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", nargs="*", default=["ml1m:1", "ml1m:50", "ml25m:50"])
    ap.add_argument("--requests", type=int, nargs="*", default=[1, 100, 10000])
    ap.add_argument("--request-shape", default="ml25m:50")
    ap.add_argument("--top-n", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    ctx = P.Context(0)
    doc = {"top_n": a.top_n, "reps": a.reps, "smoothing": "jm 0.1", "time": "ms_prepare + ms_total (HIP events)", "jobs": [], "requests": []}

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")

    for spec in a.jobs:
        shape, K = spec.split(":")[0], int(spec.split(":")[1])
        ratings, clustering, facts = load(P, S, ctx, shape, K)
        row = {"shape": shape, "clusters": K, "nnz": int(ratings.nnz)}
        for model in ("rm2", "rm1"):
            job = P.RM2Job(conf_of(P, model, facts["n_items"], K, a.top_n), ctx)
            sts = []
            for rep in range(a.reps + 1):       # (the first is the warm-up)
                rec = job.run(ratings, clustering=clustering)
                sts.append(dict(rec.stats))
                rec.close()
            row[model] = summary(sts[1:])
        rates(row["rm1"])
        row["rm1_over_rm2"] = row["rm1"]["ms_job_median"] / row["rm2"]["ms_job_median"]
        doc["jobs"].append(row)
        r1, r2 = row["rm1"], row["rm2"]
        print("job %-6s K=%-3d RM2 %10.3f ms | RM1 %12.3f ms (x%.1f) | tables %.3f lik %.3f score %.3f topn %.3f s | tested %.3e (%.3e /s) gathered %.3e (%.3e /s)"
              % (shape, K, r2["ms_job_median"], r1["ms_job_median"], row["rm1_over_rm2"], r1["ms_tables"] / 1e3, r1["ms_cooc"] / 1e3, r1["ms_score"] / 1e3,
                 r1["ms_topn"] / 1e3, r1["pair_contribs"], r1["loglik_entries_per_s"] or 0, r1["log_terms"], r1["gather_entries_per_s"] or 0), flush=True)
        flush()
        ratings.close()

    if a.requests:
        shape, K = a.request_shape.split(":")[0], int(a.request_shape.split(":")[1])
        ratings, clustering, facts = load(P, S, ctx, shape, K)
        prepared = P.RM2Job(conf_of(P, "rm1", facts["n_items"], K, a.top_n), ctx).prepare(ratings, clustering=clustering)
        order = np.random.Generator(np.random.PCG64(7)).permutation(facts["n_users"]).astype(np.int32) + 1
        for n in a.requests:
            ids = order[:n]
            sts = []
            for rep in range(a.reps + 1):
                rec = prepared.score_users(ids)
                sts.append(dict(rec.stats))
                rq = rec.request_stats
                rec.close()
            r = rates(summary(sts[1:]))
            r.update({"shape": shape, "clusters": K, "users_asked": int(n), "clusters_touched": int(rq["clusters_touched"]), "batches": int(rq["batches"])})
            doc["requests"].append(r)
            print("request %-6s K=%-3d %6d users, %3d clusters: %10.3f ms | tables %.3f lik %.3f score %.3f topn %.3f s | tested %.3e gathered %.3e"
                  % (shape, K, n, r["clusters_touched"], r["ms_total"], r["ms_tables"] / 1e3, r["ms_cooc"] / 1e3, r["ms_score"] / 1e3, r["ms_topn"] / 1e3,
                     r["pair_contribs"], r["log_terms"]), flush=True)
            flush()
        prepared.close()
        ratings.close()
    ctx.close()


if __name__ == "__main__":
    main()
