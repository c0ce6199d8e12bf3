"""The plain fp64 statement of the offline evaluation (include/filmyou.h, "offline evaluation"): the hold-out split's hash and the
ranking metrics, written from the definitions with numpy and Python loops.  No product code is used."""
import math

import numpy as np

MASK = (1 << 64) - 1
VALUES = ("hits", "recall", "ap", "rr", "ndcg")


def split_mask(user, item, fraction, seed):
    """True where (user, item) goes to the test side: (z >> 40) < floor(fraction * 2^24), z = the splitmix64 finaliser of
    ((uint32 user << 32) | uint32 item) + seed * 0x9E3779B97F4A7C15, all modulo 2^64."""
    if not 0.0 <= fraction <= 1.0:      # NaN fails both comparisons
        raise ValueError("fraction")
    threshold = int(math.floor(fraction * (1 << 24)))
    out = np.zeros(len(user), dtype=bool)
    for t, (u, i) in enumerate(zip(np.asarray(user).tolist(), np.asarray(item).tolist())):
        z = (((u & 0xFFFFFFFF) << 32) | (i & 0xFFFFFFFF)) + (int(seed) & MASK) * 0x9E3779B97F4A7C15 & MASK
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & MASK
        z = (z ^ (z >> 27)) * 0x94D049BB133111EB & MASK
        z ^= z >> 31
        out[t] = (z >> 40) < threshold
    return out


def holdout(user, item, score, fraction, seed):
    """((train user, item, score), (test user, item, score)), both in source order."""
    user, item, score = np.asarray(user, dtype=np.int32), np.asarray(item, dtype=np.int32), np.asarray(score, dtype=np.float32)
    m = split_mask(user, item, fraction, seed)
    return (user[~m], item[~m], score[~m]), (user[m], item[m], score[m])


def gain_of(kind, score):
    s = float(score)
    return {"binary": 1.0, "linear": s, "exp2": float(np.exp2(np.float64(s)) - 1.0)}[kind]


def relevant_sets(test, threshold, gain):
    """{user: {item: gain}} over the test entries with float64(score) >= threshold (NaN never)."""
    rel, seen = {}, set()
    for u, i, s in zip(np.asarray(test[0]).tolist(), np.asarray(test[1]).tolist(), np.asarray(test[2], dtype=np.float32).tolist()):
        if (u, i) in seen:
            raise ValueError("duplicate (user, item) in test")
        seen.add((u, i))
        if float(s) >= threshold:       # NaN >= x is False
            rel.setdefault(u, {})[i] = gain_of(gain, s)
    return rel


def list_metrics(items, R, N):
    """(hits, recall, AP, RR, nDCG) of one list cut at N for the relevant set R = {item: gain}, |R| > 0."""
    hits, ap, rr, dcg = 0, 0.0, 0.0, 0.0
    for p, it in enumerate(items[:N], start=1):
        if it in R:
            hits += 1
            ap += hits / p
            if rr == 0.0:
                rr = 1.0 / p
            dcg += R[it] / math.log2(p + 1)
    idcg = 0.0
    for p, g in enumerate(sorted(R.values(), reverse=True)[:min(N, len(R))], start=1):
        idcg += g / math.log2(p + 1)
    return float(hits), hits / len(R), ap / min(len(R), N), rr, dcg / idcg


def evaluate(list_user, list_item, test, cutoffs, threshold, gain="binary", coverage=False):
    """The evaluation of rows grouped by user, best first.  Returns a dict: the counters, per cutoff `hits`, `users_hit` (int) and the
    fp64 sums `recall`, `ap`, `rr`, `ndcg` over the evaluated lists in list order, `distinct_items` (None without coverage), and
    `per_user`: {"user": ids in list order, each of VALUES: lists x cutoffs, NaN where the list is not evaluated}."""
    rel = relevant_sets(test, threshold, gain)
    lu, li = np.asarray(list_user).tolist(), np.asarray(list_item).tolist()
    starts = [t for t in range(len(lu)) if t == 0 or lu[t] != lu[t - 1]] + [len(lu)]
    n_lists, nc = len(starts) - 1, len(cutoffs)
    per = {k: np.full((n_lists, nc), np.nan) for k in VALUES}
    users = np.zeros(n_lists, dtype=np.int32)
    out = {"lists": n_lists, "users_evaluated": 0, "relevant_users": len(rel), "relevant_entries": sum(len(r) for r in rel.values()),
           "hits": [0] * nc, "users_hit": [0] * nc, "recall": [0.0] * nc, "ap": [0.0] * nc, "rr": [0.0] * nc, "ndcg": [0.0] * nc}
    covered = set()
    for l in range(n_lists):
        items = li[starts[l]:starts[l + 1]]
        users[l] = lu[starts[l]]
        covered.update(items[:cutoffs[-1]])
        R = rel.get(lu[starts[l]])
        if not R:
            continue
        out["users_evaluated"] += 1
        for c, N in enumerate(cutoffs):
            vals = list_metrics(items, R, N)
            for k, v in zip(VALUES, vals):
                per[k][l, c] = v
            out["hits"][c] += int(vals[0])
            out["users_hit"][c] += vals[0] > 0
            for k, v in zip(VALUES[1:], vals[1:]):
                out[k][c] += v
    out["lists_without_relevant"] = n_lists - out["users_evaluated"]
    out["distinct_items"] = len(covered) if coverage else None
    per["user"] = users
    out["per_user"] = per
    return out
