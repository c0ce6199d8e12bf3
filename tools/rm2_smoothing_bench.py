"""The three smoothing methods of the RM2 job side by side ("Smoothing methods").

    python tools/rm2_smoothing_bench.py [--shape ml25m] [--top-n 50] [--reps 5] [--out profiles/rm2_smoothing/<name>.json]

One resident ratings object; for numberOfClusters 1 and 50, after one warm-up job of each method, `reps` rounds that alternate
Jelinek-Mercer (lambda 0.1), Dirichlet prior (mu 100) and absolute discounting (delta 0.5): a COLD job (FY_RM2_NO_CACHE: everything
built inside the job) and a WARM job (the second of two caching jobs of the method) per method and round.  Times are HIP-event
milliseconds on the context's stream, ms_prepare + ms_total of fy_stats: the whole call without the host's argument handling.
Prints one JSON document: per (clusters, method, cold | warm) the median and the spread (min, max) of the job time, the medians of
ms_prepare / ms_tables / ms_cooc / ms_score, blocks_survived / blocks_total, prune_fallbacks, and the ratio of the median job time
to Jelinek-Mercer's of the same run."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

METHODS = (("jm", "lambda", 0.1), ("dirichlet", "mu", 100.0), ("absoluteDiscounting", "delta", 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--top-n", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clusters", type=int, nargs="*", default=[1, 50])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    user, item, score, facts = S.generate(a.shape, device=torch.device("cuda", 0))
    ctx = P.Context(0)
    ratings = P.Ratings(ctx, user, item, score)
    doc = {"shape": a.shape, "top_n": a.top_n, "reps": a.reps, "nnz": int(len(score)), "time": "ms_prepare + ms_total (HIP events)", "runs": []}
    for K in a.clusters:
        clustering = None
        if K > 1:
            uu = np.arange(1, facts["n_users"] + 1, dtype=np.int32)
            clustering = (uu, S.hash_clustering(uu, K))
        jobs = {}
        for name, key, value in METHODS:
            conf = P.Configuration()
            conf.set("smoothing", name)
            conf.set(key, repr(value))
            conf.setInt("numberOfItems", facts["n_items"])
            conf.setInt("numberOfClusters", K)
            conf.setInt("numberOfRecommendations", a.top_n)
            jobs[name] = P.RM2Job(conf, ctx)

        def one(name, cache):
            rec = jobs[name].run(ratings, clustering=clustering, cache=cache)
            st = dict(rec.stats)
            rec.close()
            return st

        for name, _, _ in METHODS:          # warm-up of each
            one(name, False)
        samples = {(name, kind): [] for name, _, _ in METHODS for kind in ("cold", "warm")}
        for _ in range(a.reps):
            for name, _, _ in METHODS:
                samples[(name, "cold")].append(one(name, False))
                one(name, True)             # (re)builds the kept state for this method's key ...
                st = one(name, True)        # ... and finds it
                assert st["prepared_from_cache"] == 1
                samples[(name, "warm")].append(st)
        med = {}
        for (name, kind), sts in samples.items():
            t = np.array([x["ms_prepare"] + x["ms_total"] for x in sts])
            med[(name, kind)] = float(np.median(t))
            doc["runs"].append({
                "clusters": K, "method": name, "kind": kind, "ms_job_median": float(np.median(t)), "ms_job_min": float(t.min()),
                "ms_job_max": float(t.max()), "ms_job_all": [float(x) for x in t],
                **{k: float(np.median([x[k] for x in sts])) for k in ("ms_prepare", "ms_tables", "ms_cooc", "ms_score", "ms_topn")},
                "blocks_survived": int(sts[-1]["blocks_survived"]), "blocks_total": int(sts[-1]["blocks_total"]),
                "prune_fallbacks": int(max(x["prune_fallbacks"] for x in sts)), "recs": int(sts[-1]["recs"])})
        for r in doc["runs"]:
            if r["clusters"] == K:
                r["ratio_to_jm"] = r["ms_job_median"] / med[("jm", r["kind"])]
    ratings.close()
    ctx.close()
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    for r in doc["runs"]:
        print("K=%-3d %-20s %-4s job %8.3f ms (%.3f .. %.3f) x%.3f of JM | prepare %.3f tables %.3f cooc %.3f score %.3f | blocks %d / %d, fallbacks %d"
              % (r["clusters"], r["method"], r["kind"], r["ms_job_median"], r["ms_job_min"], r["ms_job_max"], r["ratio_to_jm"], r["ms_prepare"],
                 r["ms_tables"], r["ms_cooc"], r["ms_score"], r["blocks_survived"], r["blocks_total"], r["prune_fallbacks"]))


if __name__ == "__main__":
    main()
