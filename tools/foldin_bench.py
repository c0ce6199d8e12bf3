#!/usr/bin/env python3
"""Times the fold-in of given profiles (fy_foldin_assign) at ML-25M shape: `python tools/foldin_bench.py [--items 59047] [--k 50]
[--iterations 10] [--profile-items 150] [--reps 5] [--no-nmf] [--out profiles/foldin/ml25m.json]`.

Profiles: 1, 1 000 and 100 000 synthetic whole profiles of ~profile-items distinct items (uniform over the items, half-star scores)
on a random W; plus one second-level configuration (k parents of --parent-items items and --sub-clusters sub-clusters each) at 100 000
profiles.  One warm-up call, then `reps` timed calls per size.  Reported per size, from the same run: the medians of fy_foldin_stats'
ms_ingest / ms_level1 / ms_level2 / ms_total, the wall clock around a drained context, profiles/s (by ms_total), and GB/s of level 1
against the gather model entries x k x 8 B.  Unless --no-nmf, fy_nmf_factorize's ms_cooc per iteration at the same shape (the
synthetic ML-25M ratings, k clusters) is printed beside it: the price of the re-factorisation the fold-in avoids.
Known limit, measured here and not fixed: at k = 50 fourteen of a wave's 64 lanes idle during the gather."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_profiles(rng, n, n_items, per):
    lens = np.clip(rng.poisson(per, n), 1, n_items).astype(np.int64)
    start = np.r_[0, np.cumsum(lens)].astype(np.int64)
    # a random start and a random step modulo the item count: duplicates inside a profile are rare (and superseded by the ingest)
    first = rng.integers(0, n_items, n)
    step = rng.integers(1, n_items, n)
    owner = np.repeat(np.arange(n), lens)
    pos = np.arange(start[-1]) - start[owner]
    item = ((first[owner] + pos * step[owner]) % n_items + 1).astype(np.int32)
    score = (rng.integers(1, 11, len(item)) * 0.5).astype(np.float32)
    return (np.arange(1, n + 1, dtype=np.int32), start, item, score)


def timed(ctx, fold, profiles, iterations, reps):
    fold.assign(profiles, iterations=iterations).close()      # warm-up
    runs = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        a = fold.assign(profiles, iterations=iterations)
        ctx.synchronize()
        st = dict(a.foldin_stats, wall_ms=(time.perf_counter() - t0) * 1e3)
        a.close()
        runs.append(st)
    med = {k: float(np.median([r[k] for r in runs])) for k in ("ms_ingest", "ms_level1", "ms_level2", "ms_total", "wall_ms")}
    med.update({k: runs[0][k] for k in ("profiles_mine", "entries", "items_composed", "items_in_parent", "profiles_assigned", "launches")})
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=59047)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--profile-items", type=int, default=150)
    ap.add_argument("--parent-items", type=int, default=20000)
    ap.add_argument("--sub-clusters", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nmf-iterations", type=int, default=2)
    ap.add_argument("--no-nmf", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "foldin", "ml25m.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("foldin_bench: no GPU (there is no CPU fallback and no CPU timing)")
    P = importlib.import_module("filmyou-core_amd")
    rng = np.random.default_rng(1)
    ctx = P.Context(0)
    k = a.k
    W = rng.random((a.items, k)) + 0.01
    out = {"items": a.items, "k": k, "iterations": a.iterations, "profile_items": a.profile_items, "sizes": []}
    fold = P.FoldIn(ctx, W, ppc=True, normalizationFrequency=12)
    sets = {n: synthetic_profiles(rng, n, a.items, a.profile_items) for n in (1, 1000, 100000)}
    print("%9s %9s %9s %9s %9s %9s %12s %8s" % ("profiles", "ingest", "level1", "level2", "total", "wall", "profiles/s", "GB/s"))

    def report(label, med, model_entries, gather_ms):
        med["profiles_per_s"] = med["profiles_mine"] / (med["ms_total"] * 1e-3)
        med["gather_gb_per_s"] = model_entries * k * 8 / (gather_ms * 1e-3) / 1e9
        med["label"] = label
        out["sizes"].append(med)
        print("%9s %9.3f %9.3f %9.3f %9.3f %9.3f %12.0f %8.1f" % (label, med["ms_ingest"], med["ms_level1"], med["ms_level2"], med["ms_total"],
                                                                    med["wall_ms"], med["profiles_per_s"], med["gather_gb_per_s"]))
    for n, prof in sets.items():
        med = timed(ctx, fold, prof, a.iterations, a.reps)
        report(str(n), med, med["items_composed"], med["ms_level1"])
    # one second-level configuration: k parents, ascending random item lists, random W_c
    lists = [np.sort(rng.choice(a.items, a.parent_items, replace=False) + 1).astype(np.int32) for _ in range(k)]

    class Maps:
        items_in_cluster = np.full(k, a.parent_items, np.int32)
        item = np.concatenate(lists)
    fold.add_level(Maps, [rng.random((a.parent_items, a.sub_clusters)) + 0.01 for _ in range(k)], stride=3251)
    med = timed(ctx, fold, sets[100000], a.iterations, a.reps)
    report("100000+L2", med, med["items_composed"], med["ms_level1"])
    out["level2_gather_gb_per_s"] = med["items_in_parent"] * a.sub_clusters * 8 / (med["ms_level2"] * 1e-3) / 1e9
    print("level 2 alone: %d entries with a row in their parent, %.1f GB/s against entries x k_c x 8 B" % (med["items_in_parent"], out["level2_gather_gb_per_s"]))
    fold.close()
    if not a.no_nmf:
        S = importlib.import_module("filmyou-core_amd.synth")
        user, item, score, facts = S.generate("ml25m", device=torch.device("cuda", 0))
        n_users, n_items = int(user.max()), int(item.max())
        conf = P.Configuration()
        for key, v in (("numberOfUsers", n_users), ("numberOfItems", n_items), ("numberOfClusters", k), ("numberOfIterations", a.nmf_iterations),
                       ("normalizationFrequency", 12)):
            conf.setInt(key, v)
        R = P.Ratings(ctx, user, item, score)
        drv = P.NMFDriver(conf, ctx, ppc=True)
        try:
            drv.run(R, rng.random((n_users, k)) + 0.01, rng.random((n_items, k)) + 0.01)
            out["nmf"] = {"n_users": n_users, "n_items": n_items, "nnz": drv.stats["nnz"], "iterations": a.nmf_iterations,
                          "ms_cooc_per_iteration": drv.stats["ms_cooc"] / a.nmf_iterations, "ms_prepare": drv.stats["ms_prepare"],
                          "ms_total": drv.stats["ms_total"]}
            print("fy_nmf_factorize at the same shape (%d x %d, %d ratings): %.1f ms per iteration (ms_cooc), %.1f ms prepare, %.1f ms total" % (
                n_users, n_items, drv.stats["nnz"], out["nmf"]["ms_cooc_per_iteration"], drv.stats["ms_prepare"], drv.stats["ms_total"]))
        except RuntimeError as e:      # e.g. an id of the synthetic shape that nobody rated
            out["nmf"] = {"error": str(e)}
            print("fy_nmf_factorize:", e)
        R.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
