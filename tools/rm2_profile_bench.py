#!/usr/bin/env python3
"""Times RM2 lists for given profiles beside RM2 lists for named users on one prepared job:
`python tools/rm2_profile_bench.py [--shape ml25m] [--clusters 50] [--n 100] [--sizes 1,100,10000] [--reps 5] [--out FILE.json]`.

The ratings are put into HBM once and ONE job is prepared (users hashed to equal clusters).  Per size k, with k random users (fixed
seed), after a warm-up of every leg, `reps` rounds ALTERNATE in one run:
  users_<k>      (A) PreparedRM2.score_users of the k users: the yardstick
  resident_<k>   (B) PreparedRM2.score_profiles(base="resident") of the same users with 5 writes each: 4 items of the user's cluster
                 that the user had not rated (taken from the rows of other members) and 1 delete of an own item.  The profile call
                 should cost (A) plus the ingest
  whole_<k>      (C) PreparedRM2.score_profiles(base="whole") of k visitors with 20 items each, taken from the rows of members of a
                 random non-empty cluster, scored in that cluster
Reported per leg: every run's ms_total (HIP events on the context's stream around the whole call), its median and spread, the
per-phase medians (ms_tables: request state, p(i|C), ingest, planning; ms_cooc: slab build; ms_score; ms_topn), the share of
ms_tables, rows and the request / profile statistics.  Nothing is compared here: tests/test_rm2_profiles_gpu.py does that."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PHASES = ("ms_tables", "ms_cooc", "ms_score", "ms_topn")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--clusters", type=int, default=50)
    ap.add_argument("--n", type=int, default=100, help="numberOfRecommendations")
    ap.add_argument("--sizes", default="1,100,10000")
    ap.add_argument("--lam", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("rm2_profile_bench: no GPU (there is no CPU fallback and no CPU timing)")
    os.environ["FY_REQ_FULL_SHARE"] = "2"
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    user, item, score, facts = S.generate(a.shape, device=torch.device("cuda", 0))
    keep = score > 0
    hu, hi = user[keep].cpu().numpy(), item[keep].cpu().numpy()
    ctx = P.Context(0)
    R = P.Ratings(ctx, user, item, score)
    del user, item, score, keep
    # rows by user on the host, to make up writes that have a column in the user's cluster
    order = np.argsort(hu, kind="stable")
    hu, hi = hu[order], hi[order]
    all_users, first = np.unique(hu, return_index=True)
    all_users = all_users.astype(np.int32)
    bounds = np.r_[first, len(hu)]
    row = lambda k: hi[bounds[k]:bounds[k + 1]]
    K = a.clusters
    cl = S.hash_clustering(all_users, K)
    members = [np.flatnonzero(cl == c) for c in range(K)]
    conf = P.Configuration()
    conf.set("lambda", repr(a.lam))
    conf.setInt("numberOfItems", facts["n_items"])
    conf.setInt("numberOfClusters", K)
    conf.setInt("numberOfRecommendations", a.n)
    job = P.RM2Job(conf, ctx).prepare(R, clustering=(all_users, cl))
    rng = np.random.default_rng(a.seed)
    shuffled = rng.permutation(len(all_users))
    nonempty = [c for c in range(K) if len(members[c])]

    def others_items(c, n, own):
        got = []
        while len(got) < n:
            cand = row(int(rng.choice(members[c])))
            cand = cand[~np.isin(cand, own)]
            cand = cand[~np.isin(cand, got)]
            got += rng.permutation(cand)[: n - len(got)].tolist()
        return got

    legs = {}
    for k in [int(x) for x in a.sizes.split(",")]:
        pick = shuffled[: min(k, len(shuffled))]
        legs["users_%d" % k] = ("users", np.ascontiguousarray(all_users[pick]))
        labels, start, items, scores, remove = [], [0], [], [], []
        for u in pick.tolist():
            own = row(u)
            items += others_items(int(cl[u]), 4, own) + [int(rng.choice(own))]
            scores += [4.0] * 4 + [0.0]
            remove += [0] * 4 + [1]
            labels.append(int(all_users[u]))
            start.append(len(items))
        legs["resident_%d" % k] = ("resident", (np.array(labels, dtype=np.int32), np.array(start, dtype=np.int64), np.array(items, dtype=np.int32),
                                                np.array(scores, dtype=np.float32), np.array(remove, dtype=np.uint8)), None)
        labels, start, items, clusters = [], [0], [], []
        for v in range(len(pick)):
            c = int(rng.choice(nonempty))
            items += others_items(c, 20, np.zeros(0, dtype=hi.dtype))
            labels.append(-1 - v)
            clusters.append(c)
            start.append(len(items))
        legs["whole_%d" % k] = ("whole", (np.array(labels, dtype=np.int32), np.array(start, dtype=np.int64), np.array(items, dtype=np.int32),
                                          np.full(len(items), 3.0, dtype=np.float32)), np.array(clusters, dtype=np.int32))

    def run(leg):
        if leg[0] == "users":
            rec = job.score_users(leg[1])
            extra = rec.request_stats
        else:
            rec = job.score_profiles(leg[1], base=leg[0], clusters=leg[2])
            extra = rec.profile_stats
        st = dict(rec.stats)
        rec.close()
        return st, extra

    out = {"shape": a.shape, "facts": {k: facts[k] for k in ("n_users", "n_items", "nnz")}, "clusters": K, "number_of_recommendations": a.n,
           "lambda": a.lam, "reps": a.reps, "legs": {}}
    rec = {name: {"ms_total_runs": [], "phases": {p: [] for p in PHASES}} for name in legs}
    for leg in legs.values():
        run(leg)                                          # warm-up (the first request builds the job's kept state)
    for _ in range(a.reps):
        for name, leg in legs.items():
            st, extra = run(leg)
            r = rec[name]
            r["ms_total_runs"].append(st["ms_total"])
            for p in PHASES:
                r["phases"][p].append(st[p])
            r["scored"], r["rows"], r["stats"] = st["users_scored"], st["recs"], extra
    print("== %s, %d clusters, N = %d" % (a.shape, K, a.n), flush=True)
    for name, r in rec.items():
        t = r["ms_total_runs"]
        r["ms_total_median"], r["ms_total_min"], r["ms_total_max"] = float(np.median(t)), min(t), max(t)
        r["phases"] = {p + "_median": float(np.median(v)) for p, v in r["phases"].items()}
        r["tables_share"] = r["phases"]["ms_tables_median"] / r["ms_total_median"] if r["ms_total_median"] else 0.0
        print("%-16s %10.3f ms (%.3f .. %.3f)  tables %.3f ms = %.2f of the call  %7d lists %9d rows  %s  %s" % (
            name, r["ms_total_median"], r["ms_total_min"], r["ms_total_max"], r["phases"]["ms_tables_median"], r["tables_share"], r["scored"],
            r["rows"], " ".join("%s %.3f" % (k[3:-7], v) for k, v in r["phases"].items()), json.dumps(r["stats"])), flush=True)
    out["legs"] = rec
    job.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
