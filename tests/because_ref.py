"""The plain statement, in numpy / fp64, of named pairs explained by their contributing preferences (include/filmyou.h, "named
pairs explained by their contributing preferences").  No product code.

The explanation of (u, i) is the decomposition of the cell tests/estimate_ref.py finishes:
  kept preferences of u     estimate_ref.kept_preferences (in the order of the additions)
  a kept preference j CONTRIBUTES iff its similarity row is non-empty and holds i; it carries sim (the row's float32), pref (the
  stored float32, 1 with boolean data) and the weight (double) pref * (double) sim -- exact in fp64
  order within a pair       a NaN weight after every number, weight descending, equal weights by ascending id of the contributor
  at most how_many are listed; `contributors` counts them all; unknown users / items list none."""
import math

import numpy as np

import estimate_ref as ER

BLOCK_USERS, BLOCK_ITEMS, BLOCK_X, BLOCK_LACKS, BLOCK_TWINS = 30, 80, 17, (3, 22, 41, 60, 79), (10, 55)


def order_key(entry):
    """entry = (contributor, sim, pref, weight)"""
    j, _, _, w = entry
    return (1, 0.0, j) if math.isnan(w) else (0, -w, j)


def contributors(u, i, s, sim_item, sim_other, sim_value, users, items, max_prefs, boolean=False):
    """-> per asked pair None (unknown user or item) or ALL its contributors [(contributor, sim, pref, weight)] in the order of the
    user's preferences.  sim_value: the rows' float32 values (any float dtype holding them exactly)."""
    kept = ER.kept_preferences(u, i, s, max_prefs)
    rows = ER.similarity_rows(sim_item, sim_other, sim_value)
    known_items = set(np.unique(i).tolist())
    cache = {}
    out = []
    for x, it in zip(np.asarray(users).tolist(), np.asarray(items).tolist()):
        if x not in kept or it not in known_items:
            out.append(None)
            continue
        if x not in cache:
            cells = {}
            for j, p in kept[x]:
                pref = 1.0 if boolean else p
                for other, v in rows.get(j) or ():
                    cells.setdefault(other, []).append((j, v, pref, pref * v))
            cache[x] = cells
        out.append(cache[x].get(it, []))
    return out


def listed(all_contributors, how_many):
    """-> (rows [(pair, contributor, sim bits, pref bits)], contributors int32 [n], start int64 [n + 1]) of the call with how_many"""
    rows, cnt, start = [], [], [0]
    for t, c in enumerate(all_contributors):
        best = sorted(c or [], key=order_key)[:how_many]
        rows += [(t, j, int(np.float32(v).view(np.uint32)), int(np.float32(p).view(np.uint32))) for j, v, p, _ in best]
        cnt.append(len(c or []))
        start.append(len(rows))
    return rows, np.array(cnt, dtype=np.int32), np.array(start, dtype=np.int64)


def fold(terms, boolean=False):
    """[(sim, pref)] in the order of the user's preferences -> the estimate's float32 (the additions of the estimate, Python doubles)"""
    num = den = 0.0
    for v, p in terms:
        num += p * v
        den += abs(v)
    return np.float32(num if boolean else num / den)


def block_data():
    """30 users x 80 items, every cell rated in half stars, but: user X rates everything 4.0 and lacks five items; two items have
    identical rating columns.  With K >= 79 and no threshold every (cosine) row holds every other item, so each of X's five
    missing items has 75 contributors -- more than a wave has lanes and more than how_many can list -- two of them of equal weight."""
    rng = np.random.default_rng(23)
    A = rng.integers(1, 11, size=(BLOCK_USERS, BLOCK_ITEMS)).astype(np.float32) / 2
    a, b = BLOCK_TWINS
    A[:, b - 1] = A[:, a - 1]
    A[BLOCK_X - 1, :] = 4.0
    user, item = np.meshgrid(np.arange(1, BLOCK_USERS + 1), np.arange(1, BLOCK_ITEMS + 1), indexing="ij")
    keep = ~((user == BLOCK_X) & np.isin(item, BLOCK_LACKS))
    return user[keep].astype(np.int32), item[keep].astype(np.int32), A[keep]
