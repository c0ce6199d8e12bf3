"""The RM1 estimator of Parapar et al. 2013 over the RM2 job's neighbourhoods, stated plainly (test infrastructure: numpy fp64,
nothing of the product library is involved).

    score(u, i) = -ln U_c + ln  sum_{v in V_c, v != u}  c_vi * prod_{j in rated(u)} c_vj          i not rated by u
    c_vi        = w r'_vi / d_v + beta_v p_i                  (the table of tests/rm2_smoothing_definition.py, all three methods)

Everything else is the RM2 job's: kept ratings are score > 0, p_i = (sum of the ratings of i) / (sum over the users of floor(s_v)),
a user the map does not name goes to cluster 0, the candidates of u are the items of its cluster it has not rated, a user without a
candidate gets no list, the (float) cast, ties by ascending item id.

`definition_full` forms C densely per cluster and takes a log-sum-exp over the neighbours:

    L_uv = sum_{j in rated(u)} ln c_vj ,  m_u = max_v L_uv ,  score = -ln U_c + m_u + ln( sum_v exp(L_uv - m_u) c_vi )

`definition_sparse` is the form the GPU pass uses: e_vj = ln c_vj - ln p_j per kept rating, cnt_uv = |rated(u) & rated(v)|,
E_uv = sum of e_vj over the intersection, LP_u = sum_{j in rated(u)} ln p_j,

    L_uv = LP_u + E_uv + (n_u - cnt_uv) ln beta_v                                   (0 * -inf := 0)
    sum_v w_uv c_vi = p_i sum_v w_uv beta_v + sum_{v rates i} w_uv (w r'_vi / d_v)

tests/test_rm1_cpu.py holds the two equal, and the dense one equal to a brute-force product in extended precision."""
import numpy as np
import scipy.sparse as sp

from rm2_smoothing_definition import user_model


def _prepare(u, i, s, method, param, clustering):
    u, i, s = np.asarray(u), np.asarray(i), np.asarray(s)
    keep = s > 0
    u, i, s = u[keep].astype(np.int64), i[keep].astype(np.int64), s[keep].astype(np.float64)
    uu, ui = np.unique(u, return_inverse=True)
    iu, ii = np.unique(i, return_inverse=True)
    U, I = len(uu), len(iu)
    su = np.bincount(ui, weights=s, minlength=U)
    nu = np.bincount(ui, minlength=U).astype(np.float64)
    p = np.bincount(ii, weights=s, minlength=I) / np.floor(su).sum()
    x, beta_r, w = user_model(method, param, s, su[ui], nu[ui])
    beta = np.zeros(U)
    beta[ui] = beta_r
    cl = np.zeros(U, dtype=np.int64)
    if clustering is not None:
        mu, mc = np.asarray(clustering[0]).astype(np.int64), np.asarray(clustering[1]).astype(np.int64)
        pos = np.clip(np.searchsorted(uu, mu), 0, U - 1)
        ok = uu[pos] == mu
        cl[pos[ok]] = mc[ok]
    X = sp.csr_matrix((w * x, (ui, ii)), shape=(U, I))          # a_vi = w r'_vi / d_v (explicit zeros kept: r' = 0 is still a rating)
    Rated = sp.csr_matrix((np.ones(len(s)), (ui, ii)), shape=(U, I))
    return uu, iu, p, beta, cl, X, Rated


def _emit(parts, user, cluster, item_ids, rated_row, sc, score_dtype):
    cand = np.flatnonzero(~rated_row)
    sc32 = sc[cand].astype(score_dtype)
    order = np.lexsort((item_ids[cand], -sc32.astype(np.float64)))
    parts[0].append(np.full(len(cand), user))
    parts[1].append(item_ids[cand][order])
    parts[2].append(sc32[order])
    parts[3].append(np.full(len(cand), cluster))


def _result(parts, score_dtype):
    cat = lambda part, dt: np.concatenate(part).astype(dt) if part else np.zeros(0, dtype=dt)
    return {"rec_user": cat(parts[0], np.int32), "rec_item": cat(parts[1], np.int32), "rec_score": cat(parts[2], score_dtype),
            "rec_cluster": cat(parts[3], np.int32)}


def definition_full(u, i, s, method, param, clustering=None, score_dtype=np.float32):
    """Every candidate of every user, in the layout of rm2_smoothing_definition.definition_full (util.assert_topn_matches applies)."""
    uu, iu, p, beta, cl, X, Rated = _prepare(u, i, s, method, param, clustering)
    parts = ([], [], [], [])
    for c in np.unique(cl):
        mem = np.flatnonzero(cl == c)
        Uc = len(mem)
        items = np.flatnonzero(np.asarray(Rated[mem].sum(0)).ravel() > 0)
        C = X[mem][:, items].toarray() + np.outer(beta[mem], p[items])
        rated = Rated[mem][:, items].toarray() > 0
        with np.errstate(divide="ignore"):
            lnC = np.log(C)
        for k in range(Uc):
            J = np.flatnonzero(rated[k])
            if len(J) == len(items):
                continue                                        # no candidate left: no list
            L = lnC[:, J].sum(1)
            L[k] = -np.inf                                      # v != u
            m = L.max() if Uc else -np.inf
            if np.isfinite(m):
                with np.errstate(divide="ignore"):
                    sc = -np.log(float(Uc)) + m + np.log(np.exp(L - m) @ C)
            else:
                sc = np.full(len(items), -np.inf)               # no neighbour with a positive likelihood (or U_c = 1)
            _emit(parts, uu[mem[k]], c, iu[items], rated[k], sc, score_dtype)
    return _result(parts, score_dtype)


def definition_sparse(u, i, s, method, param, clustering=None, score_dtype=np.float32):
    """The same rows through the two sparse products."""
    uu, iu, p, beta, cl, X, Rated = _prepare(u, i, s, method, param, clustering)
    parts = ([], [], [], [])
    for c in np.unique(cl):
        mem = np.flatnonzero(cl == c)
        Uc = len(mem)
        items = np.flatnonzero(np.asarray(Rated[mem].sum(0)).ravel() > 0)
        R = Rated[mem][:, items].tocsr()
        A = X[mem][:, items].tocsr()
        R.sort_indices()
        A.sort_indices()
        assert np.array_equal(R.indptr, A.indptr) and np.array_equal(R.indices, A.indices)
        pc, bc = p[items], beta[mem]
        rows = np.repeat(np.arange(Uc), np.diff(R.indptr))
        e = np.log(A.data + bc[rows] * pc[R.indices]) - np.log(pc[R.indices])          # one log per kept rating
        E = sp.csr_matrix((e, R.indices, R.indptr), shape=R.shape)
        n = np.diff(R.indptr).astype(np.float64)
        cnt = (R @ R.T).toarray()
        Euv = (R @ E.T).toarray()                                                       # [u][v] = sum over the intersection of e_vj
        LP = R @ np.log(pc)
        with np.errstate(divide="ignore"):
            lnb = np.log(bc)
        missing = n[:, None] - cnt
        with np.errstate(invalid="ignore"):
            L = LP[:, None] + Euv + np.where(missing == 0, 0.0, missing * lnb[None, :])
        np.fill_diagonal(L, -np.inf)
        m = L.max(1) if Uc else np.zeros(0)
        live = np.isfinite(m)
        Wt = np.zeros_like(L)
        Wt[live] = np.exp(L[live] - m[live, None])
        tot = pc[None, :] * (Wt @ bc)[:, None] + (A.T @ Wt.T).T
        rated = R.toarray() > 0
        for k in range(Uc):
            if rated[k].all():
                continue
            if live[k]:
                with np.errstate(divide="ignore"):
                    sc = -np.log(float(Uc)) + m[k] + np.log(tot[k])
            else:
                sc = np.full(len(items), -np.inf)
            _emit(parts, uu[mem[k]], c, iu[items], rated[k], sc, score_dtype)
    return _result(parts, score_dtype)
