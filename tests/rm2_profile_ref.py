"""RM2 lists for given profiles and pending writes, stated plainly (test infrastructure: numpy fp64, nothing of the product library).

The prepared job is the RM2 job's own model: kept ratings are score > 0, s_v = sum of the kept ratings of v, p_i = (sum of the
ratings of i) / (sum over the users of floor(s_v)), a user the map does not name goes to cluster 0, the items of a cluster are
those somebody of the cluster rated, c_vi = (1 - lambda) r_vi / s_v + lambda p_i.  NOTHING of it follows the writes.

Composition, per profile (include/filmyou.h, fy_rm2_score_profiles):
  * "resident": the starting set is the prepared row of the labelled user and the cluster is that user's; a label the job does not
    know gets no list (users_unknown), a label < filterUsers gets no list (users_filtered); the entries of such a profile are
    counted in `entries` and not looked at.  "whole": the starting set is empty, the cluster is the one given.
  * an entry whose item has no column in the cluster is dropped and counted (entries_unknown_item);
  * the others are applied in the order given, the last entry per item counts; every earlier one is superseded;
  * a last entry that is a delete removes the item (removes_hit if the prepared row holds it, else removes_missed); a last entry
    whose score is not > 0 removes it too (entries_nonpositive); any other last entry puts the item in;
  * the composed set is listed in the cluster's rank order: most raters first, ties by ascending raw id.

Scores are DIRECT fp64 sums over the neighbours from the dense per-cluster c_vi:
    resident:  (n' - 1) ln M - n' ln U_c       + sum_{j in profile} ln  sum_{v in c, v != u} c_vi c_vj
    whole:     (n' - 1) ln M - n' ln (U_c + 1) + sum_{j in profile} ln  sum_{v in c}         c_vi c_vj
for every item i of the cluster outside the profile.  Where u is the only rater of i or of j the direct sum has no special case:
at lambda = 0 it is exactly 0 and the score -inf.  An empty profile and a profile without a candidate get no list.
"""
import numpy as np

COUNTERS = ("profiles_asked", "profiles_mine", "profiles_scored", "profiles_empty", "users_unknown", "users_filtered", "entries",
            "entries_unknown_item", "entries_nonpositive", "entries_superseded", "removes_hit", "removes_missed", "items_composed")


class Model:
    """The prepared job.  clusters[c] = dict(members (raw user ids), items (raw ids in rank order), C (U_c x I_c), rated (bool))."""

    def __init__(self, u, i, s, lam, number_of_items, clustering=None):
        u, i, s = np.asarray(u), np.asarray(i), np.asarray(s)
        keep = s > 0
        u, i, s = u[keep].astype(np.int64), i[keep].astype(np.int64), s[keep].astype(np.float64)
        self.lam, self.M = float(lam), int(number_of_items)
        uu, ui = np.unique(u, return_inverse=True)
        su = np.bincount(ui, weights=s, minlength=len(uu))
        total = np.floor(su).sum()
        cl = np.zeros(len(uu), dtype=np.int64)
        if clustering is not None:
            where = {int(a): int(b) for a, b in zip(np.asarray(clustering[0]).tolist(), np.asarray(clustering[1]).tolist())}
            cl = np.array([where.get(int(x), 0) for x in uu], dtype=np.int64)
        item_sum = {}
        for it, sc in zip(i.tolist(), s.tolist()):
            item_sum[it] = item_sum.get(it, 0.0) + sc
        self.cluster_of = {int(x): int(c) for x, c in zip(uu, cl)}
        self.clusters = {}
        for c in np.unique(cl).tolist():
            members = uu[cl == c]
            inside = np.isin(u, members)
            ids, raters = np.unique(i[inside], return_counts=True)
            order = np.lexsort((ids, -raters))
            items = ids[order]
            col = {int(it): k for k, it in enumerate(items.tolist())}
            row = {int(x): k for k, x in enumerate(members.tolist())}
            X = np.zeros((len(members), len(items)))
            for x, it, sc in zip(u[inside].tolist(), i[inside].tolist(), s[inside].tolist()):
                X[row[x], col[it]] += sc
            rated = X > 0
            X /= su[np.searchsorted(uu, members)][:, None]
            p = np.array([item_sum[int(it)] / total for it in items])
            self.clusters[c] = dict(members=members, items=items, col=col, row=row, rated=rated, C=(1.0 - self.lam) * X + self.lam * p[None, :])


def compose(model, profiles, base, clusters=None, filter_users=0, rank=0, world=1):
    """profiles: [(label, items, scores, remove or None)].  Returns ([(label, cluster, [raw items in rank order]) or None per profile of
    this rank's range], counters)."""
    n = len(profiles)
    lo, hi = n * rank // world, n * (rank + 1) // world
    c = dict.fromkeys(COUNTERS, 0)
    c["profiles_asked"], c["profiles_mine"] = n, hi - lo
    out = []
    for k in range(lo, hi):
        label, items, scores, remove = profiles[k]
        items, scores = list(items), list(scores)
        remove = [0] * len(items) if remove is None else list(remove)
        c["entries"] += len(items)
        if base == "resident":
            if label not in model.cluster_of:
                c["users_unknown"] += 1
                out.append(None)
                continue
            if label < filter_users:
                c["users_filtered"] += 1
                out.append(None)
                continue
            cl = model.cluster_of[label]
            K = model.clusters[cl]
            own = set(K["items"][K["rated"][K["row"][label]]].tolist())
        else:
            cl = int(clusters[k])
            K = model.clusters[cl]
            own = set()
        have = set(own)
        last = {}
        for e, it in enumerate(items):
            if it not in K["col"]:
                c["entries_unknown_item"] += 1
                continue
            if it in last:
                c["entries_superseded"] += 1
            last[it] = e
        for it, e in last.items():
            if remove[e]:
                c["removes_hit" if it in own else "removes_missed"] += 1
                have.discard(it)
            elif not scores[e] > 0:
                c["entries_nonpositive"] += 1
                have.discard(it)
            else:
                have.add(it)
        composed = sorted(have, key=lambda it: K["col"][it])
        c["items_composed"] += len(composed)
        c["profiles_empty"] += not composed
        out.append((label, cl, composed))
    return out, c


def score(model, composed, base, top_n=None):
    """-> (groups, rows): groups = [(label, cluster, items, float32 scores)] of the profiles that get a list, in the order given, every
    candidate best first (ties by ascending item id), cut at top_n if given; rows = the same as rec_* arrays whose rec_user is the
    GROUP'S POSITION (labels may repeat), the layout util.assert_topn_matches takes as its reference."""
    groups = []
    for entry in composed:
        if entry is None:
            continue
        label, cl, items = entry
        K = model.clusters[cl]
        Ic, Uc = len(K["items"]), len(K["members"])
        if not items or len(items) >= Ic:
            continue
        C = K["C"]
        if base == "resident":
            C = np.delete(C, K["row"][label], axis=0)
            n_members = Uc
        else:
            n_members = Uc + 1
        J = np.array([K["col"][it] for it in items])
        inner = C.T @ C[:, J] if C.shape[0] else np.zeros((Ic, len(J)))          # [i][j] = sum over the neighbours of c_vi c_vj
        with np.errstate(divide="ignore"):
            sc = (len(J) - 1) * np.log(float(model.M)) - len(J) * np.log(float(n_members)) + np.log(inner).sum(1)
        cand = np.setdiff1d(np.arange(Ic), J)
        sc32 = sc[cand].astype(np.float32)
        ids = K["items"][cand]
        order = np.lexsort((ids, -sc32.astype(np.float64)))
        if top_n is not None:
            order = order[:top_n]
        groups.append((label, cl, ids[order].astype(np.int32), sc32[order]))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    rows = {"rec_user": cat([np.full(len(g[2]), k) for k, g in enumerate(groups)], np.int32), "rec_item": cat([g[2] for g in groups], np.int32),
            "rec_score": cat([g[3] for g in groups], np.float32), "rec_cluster": cat([np.full(len(g[2]), g[1]) for g in groups], np.int32)}
    return groups, rows
