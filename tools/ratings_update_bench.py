#!/usr/bin/env python3
"""Times a batch of writes applied to resident ratings beside the only alternative, a re-upload of the merged ratings:
`python tools/ratings_update_bench.py [--shape ml25m] [--sizes 10,1000,100000] [--reps 5] [--out profiles/ratings_update/ml25m.json]`.

The ratings are put into HBM once.  Per batch size a batch is made from a fixed seed -- half replacements of stored keys, a quarter
inserts of keys that are not stored, a quarter deletes of stored keys -- and the merged ratings are formed ON THE HOST OUTSIDE THE
TIMED WINDOW (the caller's own merge is not charged to the alternative).  After one warm-up of every configuration, `reps` rounds
ALTERNATE them in one run:
  updated            Ratings.updated(batch): host batch arrays in, new object out (the call ends synchronised)
  reupload           Ratings(ctx, merged host arrays): fy_ratings_create over PCIe (pageable numpy memory, as a caller holds it)
  updated+prepare    ... followed by RM2Job.prepare on the new object (one cluster, nothing cached: a new object starts with none)
  reupload+prepare
Times are host wall-clock milliseconds around calls that end in a device synchronise.  `share_of_byte_model` of `updated` = (12 B read
+ 12 B written per source entry) / time / 8 TB/s (the HBM3E peak of MI355X_MICROARCH.md) -- a whole-call figure (batch upload, sort,
both source passes, three host round trips), not a kernel's share of peak.  Nothing is compared here: tests/test_ratings_update_gpu.py
does that."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
CONFIGS = ("updated", "reupload", "updated+prepare", "reupload+prepare")


def make_batch(u, i, n_items, k, rng):
    """k writes: k/2 replacements, k/4 inserts (items beyond the data), k/4 deletes, shuffled; distinct keys"""
    n_rep, n_del = k // 2, k // 4
    n_ins = k - n_rep - n_del
    at = rng.choice(len(u), size=n_rep + n_del, replace=False)
    bu = np.concatenate([u[at], rng.choice(np.unique(u[at]) if len(at) else u[:1], size=n_ins)])
    bi = np.concatenate([i[at], n_items + 1 + np.arange(n_ins, dtype=np.int32)])
    bs = (rng.integers(1, 11, size=k) / 2).astype(np.float32)
    br = np.zeros(k, dtype=np.uint8)
    br[n_rep:n_rep + n_del] = 1
    order = rng.permutation(k)
    return bu[order].astype(np.int32), bi[order].astype(np.int32), bs[order], br[order]


def merge_on_host(u, i, s, b):
    """the caller's merge of a batch of distinct keys: survivors in order, then the live writes"""
    key = (u.astype(np.int64) << 32) | i.astype(np.int64)
    bkey = (b[0].astype(np.int64) << 32) | b[1].astype(np.int64)
    keep = ~np.isin(key, bkey)
    live = b[3] == 0
    return (np.concatenate([u[keep], b[0][live]]), np.concatenate([i[keep], b[1][live]]), np.concatenate([s[keep], b[2][live]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--sizes", default="10,1000,100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261018)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ratings_update_bench: no GPU (there is no CPU fallback and no CPU timing)")
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    user, item, score, facts = S.generate(a.shape, device=torch.device("cuda", 0))
    u, i, s = user.cpu().numpy(), item.cpu().numpy(), score.cpu().numpy()
    ctx = P.Context(0)
    R = P.Ratings(ctx, user, item, score)
    del user, item, score
    conf = P.Configuration()
    conf.set("lambda", "0.1")
    conf.setInt("numberOfItems", facts["n_items"] + 200000)
    conf.setInt("numberOfClusters", 1)
    conf.setInt("numberOfRecommendations", 50)
    job = P.RM2Job(conf, ctx)
    nnz = len(u)
    out = {"shape": a.shape, "facts": {k: facts[k] for k in ("n_users", "n_items", "nnz")}, "reps": a.reps,
           "byte_model_bytes": 24 * nnz, "runs": {}}
    rng = np.random.default_rng(a.seed)
    for k in [int(x) for x in a.sizes.split(",")]:
        b = make_batch(u, i, facts["n_items"], k, rng)
        merged = merge_on_host(u, i, s, b)
        stats = {}

        def run(name):
            ctx.synchronize()
            t0 = time.perf_counter()
            if name.startswith("updated"):
                new = R.updated(*b)
                stats.update(new.update_stats)
            else:
                new = P.Ratings(ctx, *merged)
            if name.endswith("prepare"):
                job.prepare(new).close()
            ctx.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            new.close()
            return ms

        times = {c: [] for c in CONFIGS}
        for c in CONFIGS:
            run(c)                                            # warm-up
        for _ in range(a.reps):
            for c in CONFIGS:
                times[c].append(run(c))
        assert stats["nnz_out"] == len(merged[0]) and stats["n_replaced"] == k // 2 and stats["n_deleted"] == k // 4
        rec = {"counters": dict(stats)}
        print("== %s, %d writes (%d replaced, %d inserted, %d deleted)" % (a.shape, k, stats["n_replaced"], stats["n_inserted"], stats["n_deleted"]), flush=True)
        for c in CONFIGS:
            t = times[c]
            rec[c] = {"ms_runs": t, "ms_median": float(np.median(t)), "ms_min": min(t), "ms_spread": max(t) - min(t)}
            print("%-18s %10.3f ms median  %10.3f min  (+- %.3f)" % (c, rec[c]["ms_median"], rec[c]["ms_min"], rec[c]["ms_spread"]), flush=True)
        gbs = 24.0 * nnz / (rec["updated"]["ms_median"] * 1e-3) / 1e9
        rec["updated"]["model_gb_per_s"] = gbs
        rec["updated"]["share_of_byte_model"] = gbs / HBM_PEAK_GBS
        print("updated: %.0f GB/s of the byte model, %.3f of the HBM peak" % (gbs, gbs / HBM_PEAK_GBS), flush=True)
        out["runs"][str(k)] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
