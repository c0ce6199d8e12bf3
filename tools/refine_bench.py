#!/usr/bin/env python3
"""Times cluster refinement at ML-25M shape: `python tools/refine_bench.py [--shape ml25m] [--clusters 50] [--users-per-sub-cluster 400]
[--iterations 10] [--reps 5] [--out profiles/refine/ml25m_k50.json] [--driver]`.

  (a) batched  : one fy_cluster_refine call (ClusterRefinementJob) on the resident ratings
  (b) composed : the same work from the API without it -- host extraction of every parent's submatrix (one stable sort of the
                 kept ratings by parent, then slices), one NMFDriver.run (PPC) per parent, the sub-cluster assignment of
                 ClusterAssignmentJob.run_sub on the resulting H matrices.  Its time is reported whole and split into the host
                 extraction and the rest (uploads, launches, downloads).

Both start from the same initial matrices (the header's seed formula, restated in numpy for (b)) and are compared: the number of
users whose cluster differs is recorded.  One warm-up run each, then `reps` timed runs, ALTERNATING (a) and (b); wall clock around
a drained context.  Reported: every run, median and spread (max - min) of both, the ratio of the medians, and the launch counts
-- (a)'s is fy_refine_stats::launches; (b)'s is counted from the launch sequence of fy_nmf_factorize (21 in front of the
iterations, 10 per iteration) and fy_cluster_assign (1), per parent.  --driver adds one end-to-end RMRecommenderDriver run
(top-50) and the share of the refinement stage in it (the file is written before that run and again after it)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--clusters", type=int, default=50)
    ap.add_argument("--users-per-sub-cluster", type=int, default=400)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine", "ml25m_k50.json"))
    ap.add_argument("--driver", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("refine_bench: no GPU (there is no CPU fallback and no CPU timing)")
    import refine_ref as RR
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    user, item, score, facts = S.generate(a.shape, device=torch.device("cuda", 0))
    u, i, s = user.cpu().numpy(), item.cpu().numpy(), score.cpu().numpy()
    K, ups, iters = a.clusters, a.users_per_sub_cluster, a.iterations
    users = np.unique(u).astype(np.int32)
    parents = S.hash_clustering(users, K)
    n_users = int(users.max())
    ctx = P.Context(0)
    R = P.Ratings(ctx, user, item, score)
    conf = P.Configuration()
    for k, v in (("numberOfUsers", n_users), ("numberOfClusters", K), ("usersPerSubCluster", ups), ("numberOfIterations", iters),
                 ("normalizationFrequency", 12)):
        conf.setInt(k, v)

    def batched():
        job = P.ClusterRefinementJob(conf, ctx)
        ctx.synchronize()
        t0 = time.perf_counter()
        out = job.run(R, (users, parents), seed=a.seed)
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0), out, job

    def composed():
        ctx.synchronize()
        t0 = time.perf_counter()
        keep = np.flatnonzero(s > 0)
        cl = parents[np.searchsorted(users, u[keep])]
        order = keep[np.argsort(cl, kind="stable")]
        cut = np.searchsorted(np.sort(cl), np.arange(K + 1))
        subs = []
        for c in range(K):
            sel = order[cut[c]:cut[c + 1]]
            mu, new_u = np.unique(u[sel], return_inverse=True)
            mi, new_i = np.unique(i[sel], return_inverse=True)
            subs.append((mu, mi, (new_u + 1).astype(np.int32), (new_i + 1).astype(np.int32), s[sel]))
        t_host = time.perf_counter() - t0
        parts, launches = [], 0
        stride = -(-n_users // K)
        for c, (mu, mi, cu, ci, cs) in enumerate(subs):
            k = -(-len(mu) // ups)
            H0 = RR.initial_matrix(a.seed, c, 0, len(mu), k)
            W0 = RR.initial_matrix(a.seed, c, 1, len(mi), k)
            sub = P.Configuration()
            for key, v in (("numberOfUsers", len(mu)), ("numberOfItems", len(mi)), ("numberOfClusters", k), ("numberOfIterations", iters),
                           ("normalizationFrequency", 12)):
                sub.setInt(key, v)
            H, _ = P.NMFDriver(sub, ctx, ppc=True).run((cu, ci, cs), H0, W0)
            parts.append((c, H, mu))
            launches += 21 + 10 * iters + 1
        us, cs_, counts = [], [], np.zeros(stride * K, np.int32)
        job = P.ClusterAssignmentJob(ctx)
        for c, H, mu in parts:
            _, cc = job._assign(H, 1, c * stride, counts)
            us.append(mu)
            cs_.append(cc)
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0), (np.concatenate(us), np.concatenate(cs_), counts), launches, 1e3 * t_host

    def dump(res):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    _, out_a, job = batched()                 # warm-up of both, and the comparison of what is timed
    _, out_b, launches_b, _ = composed()
    oa, ob = np.argsort(out_a[0], kind="stable"), np.argsort(out_b[0], kind="stable")
    same_users = len(out_a[0]) == len(out_b[0]) and bool(np.array_equal(out_a[0][oa], out_b[0][ob]))
    differ = int((out_a[1][oa] != out_b[1][ob]).sum()) if same_users else -1
    ta, tb, th, stats = [], [], [], None
    for _ in range(a.reps):
        t, _, job = batched()
        ta.append(t)
        stats = job.stats
        t, _, _, t_host = composed()
        tb.append(t)
        th.append(t_host)
    rest = np.array(tb) - np.array(th)
    res = {"shape": a.shape, "facts": {k: facts[k] for k in ("n_users", "n_items", "nnz")}, "parents": K, "users_per_sub_cluster": ups,
           "iterations": iters, "reps": a.reps, "same_users": same_users, "users_differing_between_a_and_b": differ,
           "batched": {"ms_runs": ta, "ms_median": float(np.median(ta)), "ms_spread": max(ta) - min(ta), "launches": stats["launches"], "stats": stats},
           "composed": {"ms_runs": tb, "ms_median": float(np.median(tb)), "ms_spread": max(tb) - min(tb), "launches": launches_b,
                        "ms_host_extraction_runs": th, "ms_without_host_extraction_median": float(np.median(rest)),
                        "ms_without_host_extraction_spread": float(rest.max() - rest.min())},
           "ratio_composed_over_batched": float(np.median(tb) / np.median(ta)),
           "ratio_composed_without_host_extraction_over_batched": float(np.median(rest) / np.median(ta)),
           "faster_by_more_than_the_spread": bool(np.median(tb) - np.median(ta) > (max(ta) - min(ta)) + (max(tb) - min(tb)))}
    dump(res)
    if a.driver:
        dconf = P.Configuration()
        for k, v in (("numberOfUsers", n_users), ("numberOfItems", int(i.max())), ("numberOfClusters", K), ("usersPerSubCluster", ups),
                     ("numberOfIterations", iters), ("numberOfRecommendations", 50)):
            dconf.setInt(k, v)
        try:
            d = P.RMRecommenderDriver(dconf, ctx)
            ctx.synchronize()
            t0 = time.perf_counter()
            rec, (du, dc, dn) = d.run(R, seed=a.seed)
            ctx.synchronize()
            wall = 1e3 * (time.perf_counter() - t0)
            res["driver"] = {"ms_wall": wall, "ms_ppc": d.stats["ppc"]["ms_total"], "ms_refine": d.stats["refine"]["ms_total"],
                             "ms_rm2": d.stats["rm2"]["ms_total"], "refine_share_of_wall": d.stats["refine"]["ms_total"] / wall,
                             "cluster_ids": int(len(dn)), "clusters_nonempty": int((dn > 0).sum()), "recs": int(rec.size)}
        except (RuntimeError, ValueError) as e:
            res["driver"] = {"error": str(e)}
        dump(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
