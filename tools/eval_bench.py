#!/usr/bin/env python3
"""Times the offline evaluation beside what a user did before it existed:
`python tools/eval_bench.py [--shape ml25m] [--configs top50,top1000] [--reps 20] [--out profiles/eval/ml25m.json] [--table]`.

The ratings of the shape are generated in HBM, split with `Ratings.holdout(0.2, seed 1)` and, per configuration, an RM2 job runs on the
train side (top50: one cluster, 50 recommendations; top1000: 50 hash clusters, 1000 recommendations).  Timed, all in one run:
  holdout     Ratings.holdout: host wall-clock around the call (it ends synchronised), median of 5 after a warm-up
  prepare     Evaluator(ctx, test, cutoffs): the same
  evaluate    Evaluator.evaluate(result): the call's own HIP-event time (`ms` of fy_eval_sums) and the host wall-clock around it,
              median of `reps` after 3 warm-ups
  host        the alternative: `rows()` (the download of the lists, timed once: a result downloads once) plus the same metrics with
              numpy on the host (`host_evaluate` below: the vectorised form of tests/eval_ref.py, binary gain), timed once
The host sums must agree with the GPU's within 1e-9 relative (a sanity check of the tool, not a test).
`--only-evaluate` makes 5 evaluate calls per configuration and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`
for the kernels' own times.  model_bytes of the metric kernel = 4 B (the item) per row inside the last cutoff + 4 B per list head;
its GB/s needs the kernel time of such a trace (`--kernel-us top50=...,top1000=...` puts it into the table).  Nothing here is a gate."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = {"top50": (1, 50, (10, 50)), "top1000": (50, 1000, (10, 100, 1000))}      # clusters, recommendations, cutoffs
THRESHOLD = 4.0


def host_evaluate(user, item, test, cutoffs, threshold):
    """Binary-gain sums of tests/eval_ref.py with numpy on whole arrays: what a user writes after downloading the lists."""
    tu, ti, ts = test
    rel = ts.astype(np.float64) >= threshold
    rkey = np.sort((tu[rel].astype(np.uint32).astype(np.uint64) << np.uint64(32)) | ti[rel].astype(np.uint32).astype(np.uint64))
    ruser, rcount = np.unique(rkey >> np.uint64(32), return_counts=True)
    head = np.flatnonzero(np.r_[True, user[1:] != user[:-1]]) if len(user) else np.zeros(0, dtype=np.int64)
    lens = np.diff(np.r_[head, len(user)])
    lid = np.repeat(np.arange(len(head)), lens)
    pos = np.arange(len(user)) - head[lid] + 1
    key = (user.astype(np.uint32).astype(np.uint64) << np.uint64(32)) | item.astype(np.uint32).astype(np.uint64)
    at = np.searchsorted(rkey, key)
    hit = (at < len(rkey)) & (rkey[np.minimum(at, len(rkey) - 1)] == key) if len(rkey) else np.zeros(len(key), dtype=bool)
    lu = user[head].astype(np.uint32).astype(np.uint64)
    if len(ruser):
        k = np.minimum(np.searchsorted(ruser, lu), len(ruser) - 1)
        known = ruser[k] == lu
        R = np.where(known, rcount[k], 1).astype(np.float64)
    else:
        known, R = np.zeros(len(lu), dtype=bool), np.ones(len(lu))
    cum = np.cumsum(hit)
    cumhit = cum - (cum[head] - hit[head].astype(np.int64))[lid]                     # hits of the list up to and at the row
    disc = 1.0 / np.log2(np.arange(1, max(cutoffs) + 1) + 1.0)
    cdisc = np.r_[0.0, np.cumsum(disc)]
    out = {"lists": len(head), "users_evaluated": int(known.sum()), "hits": [], "recall": [], "ap": [], "rr": [], "ndcg": []}
    for N in cutoffs:
        m = hit & (pos <= N)
        hits = np.bincount(lid[m], minlength=len(head)).astype(np.float64)
        ap = np.bincount(lid[m], weights=cumhit[m] / pos[m], minlength=len(head)) / np.minimum(R, N)
        dcg = np.bincount(lid[m], weights=disc[pos[m] - 1], minlength=len(head))
        first = np.full(len(head), np.inf)
        np.minimum.at(first, lid[m], pos[m])
        idcg = cdisc[np.minimum(R, N).astype(np.int64)]
        out["hits"].append(int(hits[known].sum()))
        out["recall"].append(float((hits / R)[known].sum()))
        out["ap"].append(float(ap[known].sum()))
        out["rr"].append(float((1.0 / first)[known].sum()))
        out["ndcg"].append(float((dcg / idcg)[known].sum()))
    return out


def timed(ctx, fn, reps, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def table(out, kernel_us):
    lines = ["| lists | rows | job ms | holdout ms | prepare ms | evaluate ms (events) | evaluate ms (host clock) | rows() ms | numpy on host ms | metric kernel us | model GB/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in out["runs"].items():
        us = kernel_us.get(name)
        gbs = "%.0f" % (r["model_bytes"] / (us * 1e-6) / 1e9) if us else "not measured"
        lines.append("| %s: %d | %d | %.1f | %.2f | %.2f | %.3f | %.3f | %.1f | %.0f | %s | %s |" % (
            name, r["lists"], r["rows"], r["job_ms_total"], out["holdout_ms"], r["prepare_ms"], r["evaluate_event_ms"], r["evaluate_host_ms"],
            r["rows_download_ms"], r["host_numpy_ms"], "%.1f" % us if us else "not measured", gbs))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml25m")
    ap.add_argument("--configs", default="top50,top1000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only-evaluate", action="store_true")
    ap.add_argument("--kernel-us", default="")
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("eval_bench: no GPU (there is no CPU fallback and no CPU timing)")
    P = importlib.import_module("filmyou-core_amd")
    S = importlib.import_module("filmyou-core_amd.synth")
    user, item, score, facts = S.generate(a.shape, device=torch.device("cuda", 0))
    ctx = P.Context(0)
    R = P.Ratings(ctx, user, item, score)
    del user, item, score
    out = {"shape": a.shape, "facts": {k: facts[k] for k in ("n_users", "n_items", "nnz")}, "reps": a.reps, "threshold": THRESHOLD, "runs": {}}
    if not a.only_evaluate:
        t = timed(ctx, lambda: [x.close() for x in R.holdout(0.2, 1)], 5, 1)
        out["holdout_ms"], out["holdout_ms_runs"] = float(np.median(t)), t
        print("holdout %.3f ms median of %s" % (out["holdout_ms"], ["%.3f" % x for x in t]), flush=True)
    train, test = R.holdout(0.2, 1)
    out["train_nnz"], out["test_nnz"] = train.nnz, test.nnz
    R.close()
    test_host = test.to_host()
    uu = np.unique(train.to_host()[0])
    for name in a.configs.split(","):
        K, n_rec, cutoffs = CONFIGS[name]
        conf = P.Configuration()
        conf.set("lambda", "0.1")
        conf.setInt("numberOfItems", facts["n_items"])
        conf.setInt("numberOfClusters", K)
        conf.setInt("numberOfRecommendations", n_rec)
        clustering = (uu, S.hash_clustering(uu, K)) if K > 1 else None
        job = P.RM2Job(conf, ctx)
        job.run(train, clustering=clustering).close()             # warm-up: the timed job starts from what the first kept on `train`
        rec = job.run(train, clustering=clustering)
        E = P.Evaluator(ctx, test, cutoffs=cutoffs, relevance_threshold=THRESHOLD)
        if a.only_evaluate:
            for _ in range(5):
                E.evaluate(rec)
            rec.close()
            E.close()
            continue
        r = {"clusters": K, "recommendations": n_rec, "cutoffs": list(cutoffs), "rows": int(rec.size), "job_ms_total": rec.stats["ms_total"]}
        t = timed(ctx, lambda: P.Evaluator(ctx, test, cutoffs=cutoffs, relevance_threshold=THRESHOLD).close(), 5, 1)
        r["prepare_ms"], r["prepare_ms_runs"] = float(np.median(t)), t
        ev_ms = []
        t = timed(ctx, lambda: ev_ms.append(E.evaluate(rec).ms), a.reps, 3)
        r["evaluate_event_ms"], r["evaluate_host_ms"] = float(np.median(ev_ms[3:])), float(np.median(t))
        r["evaluate_event_ms_spread"] = float(max(ev_ms[3:]) - min(ev_ms[3:]))
        ev = E.evaluate(rec)
        r["lists"] = ev.lists
        r["gpu"] = {"users_evaluated": ev.users_evaluated, "hits": ev.hits.tolist(), "means": {k: v.tolist() for k, v in ev.means().items()}}
        t0 = time.perf_counter()
        rows = rec.rows()
        r["rows_download_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        h = host_evaluate(rows["user"], rows["item"], test_host, cutoffs, THRESHOLD)
        r["host_numpy_ms"] = (time.perf_counter() - t0) * 1e3
        assert h["lists"] == ev.lists and h["users_evaluated"] == ev.users_evaluated and h["hits"] == ev.hits.tolist(), (h["hits"], ev.hits.tolist())
        for k in ("recall", "ap", "rr", "ndcg"):
            assert np.allclose(h[k], getattr(ev, k), rtol=1e-9, atol=0.0), (k, h[k], getattr(ev, k))
        heads = np.flatnonzero(np.r_[True, rows["user"][1:] != rows["user"][:-1]])
        lens = np.diff(np.r_[heads, len(rows["user"])])
        r["model_bytes"] = int(4 * np.minimum(lens, cutoffs[-1]).sum() + 4 * len(heads))
        print("== %s: %d lists, %d rows, job %.1f ms; prepare %.3f ms; evaluate %.3f ms by events (+- %.3f), %.3f ms by the host clock; rows() %.1f ms + numpy %.0f ms"
              % (name, r["lists"], r["rows"], r["job_ms_total"], r["prepare_ms"], r["evaluate_event_ms"], r["evaluate_event_ms_spread"], r["evaluate_host_ms"],
                 r["rows_download_ms"], r["host_numpy_ms"]), flush=True)
        print("   ", r["gpu"], flush=True)
        out["runs"][name] = r
        del rows
        rec.close()
        E.close()
    if a.only_evaluate:
        return
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if a.table:
        kernel_us = {kv.split("=")[0]: float(kv.split("=")[1]) for kv in a.kernel_us.split(",") if kv}
        print(table(out, kernel_us))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
