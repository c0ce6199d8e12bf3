"""The fold-in of given profiles on standing factors, stated plainly in numpy fp64 (no product code): composition with its counters,
the H update of HComputationReducer / PPCHComputationReducer for one row with W held fixed, both levels, masks and statuses.
include/filmyou.h (fy_foldin_*) is the text this restates."""
import numpy as np

OK, EMPTY, NO_CLUSTER, EMPTY_IN_PARENT = 0, 1, 2, 3
EPS = 1e-12
DBL_MAX = np.finfo(np.float64).max


def compose(n_items, items, scores, remove=None):
    """One profile -> (ascending item ids, float32 scores, counters).  An id outside [1, n_items] is dropped first; the last entry per
    item counts; a delete or a score that is not > 0 removes the item."""
    c = dict(out_of_range=0, superseded=0, removed=0, nonpositive=0)
    last = {}
    for pos, it in enumerate(np.asarray(items).reshape(-1).tolist()):
        if it < 1 or it > n_items:
            c["out_of_range"] += 1
            continue
        if it in last:
            c["superseded"] += 1
        last[it] = pos
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    kept = []
    for it in sorted(last):
        pos = last[it]
        if remove is not None and remove[pos]:
            c["removed"] += 1
        elif not scores[pos] > 0:
            c["nonpositive"] += 1
        else:
            kept.append((it, scores[pos]))
    return np.array([k[0] for k in kept], dtype=np.int64), np.array([k[1] for k in kept], dtype=np.float32), c


def clamp(v):
    v = np.array(v, dtype=np.float64)
    v[np.isposinf(v)] = DBL_MAX
    v[np.isneginf(v)] = -DBL_MAX
    return v


def update(h, x, C, ppc, normalize):
    """One multiplicative update of the row h with x = the row of A W and C = W^T W held."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        y = C @ h
        if ppc:
            d, e = h @ y, h @ x
            h = h * (clamp(x + d) / (clamp(y + e) + EPS))
            if normalize:
                h = h / np.abs(h).sum()
        else:
            h = h * (x / (y + EPS))
    return h


def fold(W, rows, scores, iterations, first_iteration, ppc, f, h0=None, C=None):
    """rows: rows of W (0-based) of the composed entries, scores their values; returns the factor row."""
    W = np.asarray(W, dtype=np.float64)
    k = W.shape[1]
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.zeros(k)
        for r, a in zip(rows, scores):
            x = x + np.float64(a) * W[r]
        C = W.T @ W if C is None else C
    h = np.full(k, 1.0 / k) if h0 is None else np.array(h0, dtype=np.float64)
    for it in range(first_iteration, first_iteration + iterations):
        # C remainder: the sign of the dividend; it >= 0, so it % f == 0 exactly when |f| divides it
        normalize = bool(ppc) and f != 0 and it % abs(f) == 0
        h = update(h, x, C, ppc, normalize)
    return h


def argmax_allowed(h, allowed=None):
    """first index of the strictly largest allowed value; NaN never wins; -1 when nothing exceeds -infinity"""
    best, mx = -1, -np.inf
    for j, v in enumerate(h):
        if (allowed is None or allowed[j]) and v > mx:
            best, mx = j, v
    return best


def margin(h, allowed=None):
    """relative gap between the two largest allowed values (inf with fewer than two comparable values)"""
    v = np.array([x for j, x in enumerate(h) if (allowed is None or allowed[j]) and not np.isnan(x)], dtype=np.float64)
    if len(v) < 2:
        return np.inf
    v = np.sort(v)[::-1]
    if v[0] == v[1]:
        return 0.0
    return abs(v[0] - v[1]) / max(abs(v[0]), abs(v[1]))


def masks(k, counts=None, level=None):
    """(allowed top-level columns or None, per-parent allowed sub-clusters or None)"""
    top = None if counts is None else [j < len(counts) and counts[j] > 0 for j in range(k)]
    sub = None
    if level is not None and level.get("counts") is not None:
        cnt, stride = level["counts"], level["stride"]
        sub = [[c * stride + j < len(cnt) and cnt[c * stride + j] > 0 for j in range(Wc.shape[1])] for c, Wc in enumerate(level["W"])]
        top = [any(s) for s in sub]
    return top, sub


def assign(W, profiles, iterations=10, first_iteration=1, ppc=True, f=-1, h0=None, counts=None, level=None):
    """profiles: [(label, items, scores[, remove])].  level: dict(items=[ascending raw ids per parent], W=[W_c], stride=, counts= or None).
    Returns a dict of arrays / lists in profile order plus the summed counters."""
    W = np.asarray(W, dtype=np.float64)
    n_items, k = W.shape
    top, sub = masks(k, counts, level)
    with np.errstate(over="ignore", invalid="ignore"):
        C = W.T @ W
        C1 = None if level is None else [np.asarray(Wc, dtype=np.float64).T @ np.asarray(Wc, dtype=np.float64) for Wc in level["W"]]
    out = dict(labels=[], clusters=[], parents=[], status=[], H=[], H1=[], margin=[], margin1=[],
               counters=dict(out_of_range=0, superseded=0, removed=0, nonpositive=0, composed=0, in_parent=0, collisions=0))
    for p, prof in enumerate(profiles):
        items, scores, c = compose(n_items, prof[1], prof[2], prof[3] if len(prof) > 3 else None)
        for key, v in c.items():
            out["counters"][key] += v
        out["counters"]["composed"] += len(items)
        h = fold(W, items - 1, scores, iterations, first_iteration, ppc, f, None if h0 is None else h0[p], C)
        a = argmax_allowed(h, top)
        status, parent, cluster, h1, m1 = OK, a, a, np.zeros(0), np.inf
        if len(items) == 0:
            status, parent, cluster = EMPTY, -1, -1
        elif a < 0:
            status, parent, cluster = NO_CLUSTER, -1, -1
        elif level is not None:
            lst, Wc = np.asarray(level["items"][a]), np.asarray(level["W"][a], dtype=np.float64)
            pos = np.searchsorted(lst, items)
            hit = (pos < len(lst)) & (lst[np.minimum(pos, max(len(lst) - 1, 0))] == items) if len(lst) else np.zeros(len(items), bool)
            out["counters"]["in_parent"] += int(hit.sum())
            h1 = fold(Wc, pos[hit], scores[hit], iterations, first_iteration, ppc, f, None, C1[a]) if Wc.shape[1] else np.zeros(0)
            a1 = argmax_allowed(h1, None if sub is None else sub[a])
            m1 = margin(h1, None if sub is None else sub[a])
            if not hit.any():
                status, cluster = EMPTY_IN_PARENT, -1
            elif a1 < 0:
                status, parent, cluster = NO_CLUSTER, -1, -1
            else:
                cluster = a * level["stride"] + a1
                out["counters"]["collisions"] += int(a1 >= level["stride"])
        out["labels"].append(prof[0]); out["clusters"].append(cluster); out["parents"].append(parent); out["status"].append(status)
        out["H"].append(h); out["H1"].append(h1); out["margin"].append(margin(h, top)); out["margin1"].append(m1)
    for key in ("labels", "clusters", "parents", "status"):
        out[key] = np.array(out[key], dtype=np.int64)
    out["H"] = np.array(out["H"]).reshape(len(profiles), k)
    return out


def profiles_of_columns(A):
    """A: items x users (the golden layout) -> one whole profile per user column: (label = user id, items, scores)"""
    A = np.asarray(A)
    out = []
    for j in range(A.shape[1]):
        rows = np.flatnonzero(A[:, j] > 0)
        out.append((j + 1, rows + 1, A[rows, j].astype(np.float32)))
    return out
