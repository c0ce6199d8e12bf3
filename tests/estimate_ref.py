"""The plain statement, in numpy / fp64, of estimated preferences for named pairs and of their error sums (include/filmyou.h,
"estimated preferences for named pairs").  No product code.

estimate(u, i) is the cell (u, i) of the item-based list pass before the top-N:
  kept preferences of u   p >= the max_prefs-th largest of u's values (all when u has no more than that; ties at the cut kept)
  a kept preference j contributes to (u, i) iff the similarity row of j holds i:  num += pref * sim, den += |sim|, cnt += 1
  (pref = 1 with boolean data), in the order of the user's preferences (popularity rank of the item: most rated first, ties by id)
  a kept preference whose row is EMPTY adds nothing, not even its self entry
status, the first that applies: 1 unknown user, 2 unknown item, 3 the item is a kept preference of the user (with a row),
4 cnt < 2 (< 1 boolean), 5 num == 0, 6 the value is NaN, else 0 with value num / den (num with boolean data)."""
import math

import numpy as np

OK, UNKNOWN_USER, UNKNOWN_ITEM, OWN_PREFERENCE, TOO_FEW, ZERO_NUMERATOR, NOT_A_NUMBER = range(7)


def kept_preferences(u, i, s, max_prefs):
    """{user: [(item, value)] in the order of the additions}"""
    ids, counts = np.unique(i, return_counts=True)
    rank = {int(it): r for r, it in enumerate(sorted(ids.tolist(), key=lambda x: (-int(counts[np.searchsorted(ids, x)]), x)))}
    out = {}
    for x in np.unique(u).tolist():
        m = u == x
        it, p = i[m], s[m]
        if len(p) > max_prefs:
            keep = p >= np.sort(p)[::-1][max_prefs - 1]
            it, p = it[keep], p[keep]
        order = sorted(range(len(it)), key=lambda k: rank[int(it[k])])
        out[int(x)] = [(int(it[k]), float(p[k])) for k in order]
    return out


def similarity_rows(sim_item, sim_other, sim_value):
    rows = {}
    for a, b, v in zip(np.asarray(sim_item).tolist(), np.asarray(sim_other).tolist(), np.asarray(sim_value, dtype=np.float64).tolist()):
        rows.setdefault(a, []).append((b, v))
    return rows


def user_cells(prefs, rows, boolean):
    """-> ({item: [num, den, cnt]}, {own items}) of one user"""
    cells, own = {}, set()
    for j, p in prefs:
        row = rows.get(j)
        if not row:
            continue
        pd = 1.0 if boolean else p
        for other, v in row:
            c = cells.setdefault(other, [0.0, 0.0, 0])
            c[0] += pd * v
            c[1] += abs(v)
            c[2] += 1
        own.add(j)
    return cells, own


def estimate(u, i, s, sim_item, sim_other, sim_value, users, items, max_prefs, boolean=False):
    """-> (value float64 [n], status int32 [n]) of the asked pairs; value is NaN unless status == OK"""
    kept = kept_preferences(u, i, s, max_prefs)
    rows = similarity_rows(sim_item, sim_other, sim_value)
    known_items = set(np.unique(i).tolist())
    cache = {}
    value = np.full(len(users), np.nan)
    status = np.zeros(len(users), dtype=np.int32)
    for t, (x, it) in enumerate(zip(np.asarray(users).tolist(), np.asarray(items).tolist())):
        if x not in kept:
            status[t] = UNKNOWN_USER
            continue
        if it not in known_items:
            status[t] = UNKNOWN_ITEM
            continue
        if x not in cache:
            cache[x] = user_cells(kept[x], rows, boolean)
        cells, own = cache[x]
        num, den, cnt = cells.get(it, (0.0, 0.0, 0))
        if it in own:
            status[t] = OWN_PREFERENCE
        elif cnt < (1 if boolean else 2):
            status[t] = TOO_FEW
        elif num == 0.0:
            status[t] = ZERO_NUMERATOR
        else:
            v = num if boolean else num / den
            if math.isnan(float(np.float32(v))):
                status[t] = NOT_A_NUMBER
            else:
                value[t] = v
    return value, status


def row_entries_walked(u, i, s, sim_item, users, items, max_prefs, chunk):
    """sum over the known asked users of (chunks of the user's distinct known asked items) x (entries of the rows of the user's kept preferences)"""
    kept = kept_preferences(u, i, s, max_prefs)
    row_len = {}
    for a in np.asarray(sim_item).tolist():
        row_len[a] = row_len.get(a, 0) + 1
    known_items = set(np.unique(i).tolist())
    targets = {}
    for x, it in zip(np.asarray(users).tolist(), np.asarray(items).tolist()):
        if x in kept and it in known_items:
            targets.setdefault(x, set()).add(it)
    return sum(-(-len(t) // chunk) * sum(row_len.get(j, 0) for j, _ in kept[x]) for x, t in targets.items())


def errors(estimate32, status, truth32, clamp=None):
    """-> counters and the per-pair terms (lists of Python floats, row order) of fy_eval_estimates: e = (double) estimate (clamped) -
    (double) truth over the OK rows with a finite truth score"""
    est = np.asarray(estimate32, dtype=np.float32).astype(np.float64)
    truth = np.asarray(truth32, dtype=np.float32).astype(np.float64)
    status = np.asarray(status)
    ok = status == OK
    finite = np.isfinite(truth)
    use = ok & finite
    e = est[use]
    if clamp is not None:
        e = np.clip(e, clamp[0], clamp[1])
    e = e - truth[use]
    return {"pairs": len(status), "estimated": int(use.sum()), "truth_not_finite": int((ok & ~finite).sum()),
            "by_status": [int((status == q).sum()) for q in range(8)],
            "abs": np.abs(e).tolist(), "sq": (e * e).tolist(), "err": e.tolist()}


def sum_bound(terms):
    """4 n 2^-53 sum |term|: the error bound of n ordered fp64 additions, with slack 4"""
    return 4.0 * len(terms) * 2.0 ** -53 * math.fsum(abs(x) for x in terms)
