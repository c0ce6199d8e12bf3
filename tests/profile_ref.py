"""The plain statement, in numpy / fp64, of item-based lists for given profiles (include/filmyou.h, "lists for given profiles and
pending writes").  No product code.

Composition of one profile: the entries (item, score, remove) are applied in the order given on top of a starting row -- the
resident user's whole row, or nothing; an entry whose item nobody rated in the prepared ratings (or whose id is negative) is dropped
and counted first; then the last entry per item counts: a write sets the preference, a delete takes the item out.  The composed
profile is ordered by the popularity rank of the item in the PREPARED ratings (most rated first, ties by ascending id).

Lists: the kept preferences of a composed profile are those >= its max_prefs-th largest value (all when it has no more than that);
a kept preference j with a non-empty similarity row adds pref * sim / |sim| / 1 to the cell of every item of the row, in the order of
the composed profile, and takes j itself out; a cell becomes a prediction when it has at least two contributions (one with boolean
data), a non-zero numerator and a value that is no NaN; the list is the predictions, best first."""
import math

import numpy as np

COUNTERS = ("profiles_asked", "profiles_mine", "profiles_empty", "users_unknown", "entries", "entries_unknown_item",
            "entries_superseded", "removes_hit", "removes_missed", "prefs_composed")


def popularity_rank(item):
    """{raw item: rank} over the prepared ratings' item column"""
    ids, counts = np.unique(np.asarray(item), return_counts=True)
    order = sorted(range(len(ids)), key=lambda k: (-int(counts[k]), int(ids[k])))
    return {int(ids[k]): r for r, k in enumerate(order)}


def compose_one(row, entries, rank):
    """row: [(item, value)] the starting row; entries: [(item, score, remove)] in order -> ([(item, float32 value)] in rank order,
    counters of this profile)"""
    c = dict(entries=len(entries), entries_unknown_item=0, entries_superseded=0, removes_hit=0, removes_missed=0)
    state = {int(i): np.float32(v) for i, v in row}
    in_row = set(state)
    last = {}
    for it, sc, gone in entries:
        it = int(it)
        if it < 0 or it not in rank:
            c["entries_unknown_item"] += 1
            continue
        if it in last:
            c["entries_superseded"] += 1
        last[it] = (np.float32(sc), bool(gone))
    for it, (sc, gone) in last.items():
        if gone:
            c["removes_hit" if it in in_row else "removes_missed"] += 1
            state.pop(it, None)
        else:
            state[it] = sc
    return sorted(state.items(), key=lambda kv: rank[kv[0]]), c


def compose(u, i, s, profiles, base, lo=0, hi=None):
    """The prepared ratings (u, i, s) and profiles [(label, items, scores, remove or None)] -> (composed [(label, [(item, value)])] of the
    profiles lo .. hi, counters as fy_itemcf_profile_stats counts them)"""
    assert base in ("whole", "resident")
    hi = len(profiles) if hi is None else hi
    rank = popularity_rank(i)
    total = dict.fromkeys(COUNTERS, 0)
    total["profiles_asked"] = len(profiles)
    total["profiles_mine"] = hi - lo
    out = []
    for label, items, scores, remove in profiles[lo:hi]:
        remove = [0] * len(items) if remove is None else remove
        row = []
        if base == "resident":
            m = np.asarray(u) == label
            if m.any():
                row = list(zip(np.asarray(i)[m].tolist(), np.asarray(s)[m].tolist()))
            else:
                total["users_unknown"] += 1
        prefs, c = compose_one(row, list(zip(items, scores, remove)), rank)
        for k, v in c.items():
            total[k] += v
        total["profiles_empty"] += not prefs
        total["prefs_composed"] += len(prefs)
        out.append((int(label), [(it, float(v)) for it, v in prefs]))
    return out, total


def similarity_rows(sim_item, sim_other, sim_value):
    rows = {}
    for a, b, v in zip(np.asarray(sim_item).tolist(), np.asarray(sim_other).tolist(), np.asarray(sim_value, dtype=np.float64).tolist()):
        rows.setdefault(a, []).append((b, v))
    return rows


def kept(prefs, max_prefs):
    if len(prefs) <= max_prefs:
        return list(prefs)
    cut = sorted((v for _, v in prefs), reverse=True)[max_prefs - 1]
    return [(it, v) for it, v in prefs if v >= cut]


def one_list(prefs, rows, max_prefs, boolean, allow=None):
    """-> [(item, float32 prediction as a Python float)] best first, every prediction (no top-N cut)"""
    num, den, cnt, own = {}, {}, {}, set()
    for j, p in kept(prefs, max_prefs):
        row = rows.get(j)
        if not row:
            continue
        pd = 1.0 if boolean else p
        for other, v in row:
            num[other] = num.get(other, 0.0) + pd * v
            den[other] = den.get(other, 0.0) + abs(v)
            cnt[other] = cnt.get(other, 0) + 1
        own.add(j)
    out = []
    for it, nm in num.items():
        if it in own or cnt[it] < (1 if boolean else 2) or nm == 0.0 or (allow is not None and it not in allow):
            continue
        v = float(np.float32(nm if boolean else nm / den[it]))
        if not math.isnan(v):
            out.append((it, v))
    out.sort(key=lambda kv: -kv[1])
    return out


def lists(composed, sim_item, sim_other, sim_value, max_prefs, boolean=False, allow=None):
    """composed: [(label, [(item, value)])] with distinct labels -> {"user", "item", "score"} of every prediction, grouped by profile in the
    order given, best first"""
    rows = similarity_rows(sim_item, sim_other, sim_value)
    allow = None if allow is None else set(np.asarray(allow).tolist())
    user, item, score = [], [], []
    for label, prefs in composed:
        for it, v in one_list(prefs, rows, max_prefs, boolean, allow):
            user.append(label); item.append(it); score.append(v)
    return {"user": np.array(user, dtype=np.int32), "item": np.array(item, dtype=np.int32), "score": np.array(score, dtype=np.float64)}
