#!/usr/bin/env python3
"""Times the recommendation pass of the item-based job for requests of different sizes: `python tools/itemcf_filter_bench.py
[--shape ml25m] [--n 100] [--k 100] [--max-prefs 50] [--reps 7] [--out profiles/itemcf/filter_ml25m.json]`.

The similarity matrix of a `synth` shape is built ONCE and stays resident, like the ratings.  Then, one warm-up run each and `reps`
timed runs, ALTERNATING the configurations:
  full            every user through the unrestricted fy_itemcf_recommend (the pass as it was before requests existed)
  items_half      every user, allow-list = half of the catalogue (fixed seed)
  users_1 / users_10 / users_100                a request of 1 % / 10 % / 100 % of the users (fixed seed, shuffled), every item
  users_1_items_half / ... / users_100_items_half   the same requests with the allow-list
Reported per configuration: every run's whole-pass time (fy_stats ms_total: HIP events on the context's stream around the pass,
from the structure of the ratings to the compacted rows), its median and spread (max - min), the per-phase medians of the
restricted pass (ms_prepare: structure of the ratings; ms_tables: similarity rows by column + the request's list and bitmap;
ms_score: accumulate + predictions; ms_topn), users that received a list, rows, and rows / s from the median.  `vs_full` is the
median over the median of `full`.  Nothing is compared here -- tests/test_itemcf_filter_gpu.py does that."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PHASES = ("ms_prepare", "ms_tables", "ms_score", "ms_topn")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--n", type=int, default=100, help="numRecommendations")
    ap.add_argument("--k", type=int, default=100, help="maxSimilaritiesPerItem")
    ap.add_argument("--max-prefs", type=int, default=50, help="maxPrefsPerUser")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=20260104)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("itemcf_filter_bench: no GPU (there is no CPU fallback and no CPU timing)")
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    user, item, score, facts = S.generate(a.shape, device=torch.device("cuda", 0))
    all_users = torch.unique(user).cpu().numpy().astype(np.int32)
    all_items = torch.unique(item).cpu().numpy().astype(np.int32)
    ctx = P.Context(0)
    R = P.Ratings(ctx, user, item, score)
    del user, item, score
    sims = P.RowSimilarityJob(ctx).run(R, maxSimilaritiesPerRow=a.k)
    rng = np.random.default_rng(a.seed)
    half = np.ascontiguousarray(rng.permutation(all_items)[: len(all_items) // 2])
    shuffled = np.ascontiguousarray(rng.permutation(all_users))
    requests = {"1": shuffled[: max(1, len(shuffled) // 100)], "10": shuffled[: max(1, len(shuffled) // 10)], "100": shuffled}
    configs = {"full": None, "items_half": (None, half)}
    for name, ids in requests.items():
        configs["users_" + name] = (ids, None)
    for name, ids in requests.items():
        configs["users_%s_items_half" % name] = (ids, half)
    lib = P._native.load()
    prm = P._native.ItemCFParams(a.n, a.max_prefs, 0, 0, 1, 0)

    def run(cfg):
        res = C.c_void_p()
        if cfg is None:
            rc = lib.fy_itemcf_recommend(ctx._h, C.byref(prm), R._h, sims._h, C.byref(res))
        else:
            u, i = cfg
            f = P._native.ItemCFFilter(int(u is not None), int(i is not None), 0 if u is None else len(u), None if u is None else u.ctypes.data,
                                       0 if i is None else len(i), None if i is None else i.ctypes.data)
            rc = lib.fy_itemcf_recommend_filtered(ctx._h, C.byref(prm), C.byref(f), R._h, sims._h, C.byref(res))
        if rc != 0:
            sys.exit("itemcf_filter_bench: %s" % lib.fy_last_error().decode(errors="replace"))
        rec = P.ItemRecommendations(res, ctx)
        st = dict(rec.stats)
        rec.close()
        return st

    out = {"shape": a.shape, "facts": {k: facts[k] for k in ("n_users", "n_items", "nnz")}, "num_recommendations": a.n,
           "max_similarities_per_item": a.k, "max_prefs_per_user": a.max_prefs, "reps": a.reps, "similarity_rows": sims.size,
           "similarity_build_ms": sims.stats["ms_total"], "configs": {}}
    rec = {name: {"requested_users": None if cfg is None or cfg[0] is None else len(cfg[0]),
                  "allowed_items": None if cfg is None or cfg[1] is None else len(cfg[1]), "ms_total_runs": [], "phases": {p: [] for p in PHASES}}
           for name, cfg in configs.items()}
    for name, cfg in configs.items():
        run(cfg)                                              # warm-up
    for _ in range(a.reps):
        for name, cfg in configs.items():
            st = run(cfg)
            r = rec[name]
            r["ms_total_runs"].append(st["ms_total"])
            for p in PHASES:
                r["phases"][p].append(st[p])
            r["users_scored"], r["rows"] = st["users_scored"], st["recs"]
    full = float(np.median(rec["full"]["ms_total_runs"]))
    for name, r in rec.items():
        t = r["ms_total_runs"]
        r["ms_total_median"] = float(np.median(t))
        r["ms_total_spread"] = max(t) - min(t)
        r["phases"] = {p + "_median": float(np.median(v)) for p, v in r["phases"].items()}
        r["rows_per_s"] = r["rows"] / (1e-3 * r["ms_total_median"])
        r["vs_full"] = r["ms_total_median"] / full
        print("%-22s %9.3f ms (+- %.3f)  x%.3f of full  %9d users %10d rows  %.3e rows/s  %s" % (
            name, r["ms_total_median"], r["ms_total_spread"], r["vs_full"], r["users_scored"], r["rows"], r["rows_per_s"],
            " ".join("%s %.3f" % (k[3:-7], v) for k, v in r["phases"].items())), flush=True)
    out["configs"] = rec
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
