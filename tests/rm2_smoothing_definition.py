"""RM2 with the three standard smoothings of the user language model, stated plainly (test infrastructure: numpy / torch fp64,
nothing of the product library is involved).

    score(u, i) = (n_u - 1) ln M - n_u ln U_c + sum_{j in rated(u)} ln( sum_{v in V_c, v != u} c_vi c_vj )     i not rated by u
    c_vi        = w r'_vi / d_v + beta_v p_i

    method                 parameter   r'_vi              d_v        beta_v            w
    "jm"                   lambda      r_vi               s_v        lambda            1 - lambda      (the reference's estimator)
    "dirichlet"            mu          r_vi               s_v + mu   mu / (s_v + mu)   1
    "absoluteDiscounting"  delta       max(r_vi - d, 0)   s_v        d n_v / s_v       1

s_v = the user's rating sum, n_v = the number of its kept ratings (score > 0), p_i = (sum of the ratings of i) / (sum over the users of
floor(s_v)) -- the reference's p(i|C) with its counter quirk -- and M = numberOfItems of the configuration.  A kept rating stays a
rated item whatever r' is: it is no candidate, and it contributes a log term.

`definition_full` forms c densely per cluster and scores every candidate of every user: C^T C minus the user's own outer product,
no identity.  `definition_rows` scores the given rows alone through the three-term identity

    sum_{v != u} c_vi c_vj = w^2 G[j][i] + p_j b~_i + p_i e~_uj ,   G = X^T X,  x = r' / d,  b~_i = w sum_v beta_v x_vi,
    e~_uj = (b~_j - w beta_u x_uj) + p_j (S2 - beta_u^2),  S2 = sum_{v in V_c} beta_v^2

for shapes whose dense matrices are too large; tests/test_rm2_smoothing_cpu.py holds the two equal."""
import numpy as np
import scipy.sparse as sp
import torch

METHODS = ("jm", "dirichlet", "absoluteDiscounting")


def _method(method):
    for m in METHODS:
        if m.lower() == str(method).lower():
            return m
    raise ValueError(method)


def user_model(method, param, r, s_of_rating, n_of_rating):
    """Per rating: (x = r' / d, beta of its user); and w.  Works on numpy arrays and torch tensors alike."""
    method = _method(method)
    if method == "jm":
        return r / s_of_rating, 0 * s_of_rating + param, 1.0 - param
    if method == "dirichlet":
        d = s_of_rating + param
        return r / d, param / d, 1.0
    rp = (r - param) * (r > param)
    return rp / s_of_rating, param * n_of_rating / s_of_rating, 1.0


def definition_full(u, i, s, method, param, number_of_items, clustering=None, score_dtype=np.float32):
    """Every candidate of every user, in the layout of oracle.rm2's result: rec_user / rec_item / rec_score (float32, like the
    reference's (float) cast) / rec_cluster, per user best first, ties by ascending item id.  clustering = (users, clusters) or None
    (everybody in cluster 0; a user the map does not name -> 0).  score_dtype=np.float64 keeps the unrounded scores."""
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
    X = sp.csr_matrix((x, (ui, ii)), shape=(U, I))
    X.sort_indices()
    Rated = sp.csr_matrix((np.ones(len(s)), (ui, ii)), shape=(U, I))
    Rated.sort_indices()
    ou, oi, osc, oc = [], [], [], []
    lnM = np.log(float(number_of_items))
    for c in np.unique(cl):
        mem = np.flatnonzero(cl == c)
        Uc = len(mem)
        items = np.flatnonzero(np.asarray(Rated[mem].sum(0)).ravel() > 0)
        C = w * X[mem][:, items].toarray() + np.outer(beta[mem], p[items])
        rated = Rated[mem][:, items].toarray() > 0
        CtC = C.T @ C
        for k in range(Uc):
            J = np.flatnonzero(rated[k])
            n = len(J)
            if n == len(items):
                continue                                    # no candidate left: no list
            inner = np.maximum(CtC[J, :] - np.outer(C[k, J], C[k, :]), 0.0)
            with np.errstate(divide="ignore"):
                sc = (n - 1) * lnM - n * np.log(float(Uc)) + np.log(inner).sum(0)
            cand = np.flatnonzero(~rated[k])
            sc32 = sc[cand].astype(score_dtype)
            order = np.lexsort((iu[items[cand]], -sc32.astype(np.float64)))
            ou.append(np.full(len(cand), uu[mem[k]]))
            oi.append(iu[items[cand]][order])
            osc.append(sc32[order])
            oc.append(np.full(len(cand), c))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return {"rec_user": cat(ou, np.int32), "rec_item": cat(oi, np.int32), "rec_score": cat(osc, score_dtype), "rec_cluster": cat(oc, np.int32)}


def definition_rows(triples, rows, method, param, number_of_items, clustering=None, device="cpu", elem_budget=1 << 24, col_chunk=2048):
    """The score of every given row (rows = dict(user, item[, cluster]) of numpy arrays), float64, through the three-term identity;
    torch fp64 on `device`.  triples = (user, item, score) as numpy arrays or torch tensors, raw ids."""
    dev = torch.device(device)
    f64 = torch.float64
    u, i, s = (torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).to(dev) for t in triples)
    keep = s > 0
    u, i, s = u[keep].long(), i[keep].long(), s[keep].to(f64)
    uid, ux = torch.unique(u, return_inverse=True)
    iid, ix = torch.unique(i, return_inverse=True)
    U, I = len(uid), len(iid)
    su = torch.zeros(U, dtype=f64, device=dev).index_add_(0, ux, s)
    n_u = torch.bincount(ux, minlength=U)
    p = torch.zeros(I, dtype=f64, device=dev).index_add_(0, ix, s) / torch.floor(su).sum()
    x, beta_r, w = user_model(method, param, s, su[ux], n_u[ux].to(f64))
    beta = torch.zeros(U, dtype=f64, device=dev)
    beta[ux] = beta_r
    cl_u = torch.zeros(U, dtype=torch.long, device=dev)
    if clustering is not None:
        mu = torch.as_tensor(np.asarray(clustering[0]), device=dev).long()
        mc = torch.as_tensor(np.asarray(clustering[1]), device=dev).long()
        pos = torch.searchsorted(uid, mu).clamp_(max=U - 1)
        ok = uid[pos] == mu
        cl_u[pos[ok]] = mc[ok]
    order = torch.argsort(ux, stable=True)
    csr_i, csr_x = ix[order], x[order]
    rowptr = torch.zeros(U + 1, dtype=torch.long, device=dev)
    rowptr[1:] = torch.cumsum(n_u, 0)

    r_user = torch.as_tensor(np.asarray(rows["user"]), device=dev).long()
    r_item = torch.as_tensor(np.asarray(rows["item"]), device=dev).long()
    r_ux = torch.searchsorted(uid, r_user)
    r_ix = torch.searchsorted(iid, r_item)
    assert bool((uid[r_ux] == r_user).all()) and bool((iid[r_ix] == r_item).all())
    r_cl = cl_u[r_ux]
    if "cluster" in rows:
        assert bool((torch.as_tensor(np.asarray(rows["cluster"]), device=dev).long() == r_cl).all()), "cluster column"
    ref = torch.empty(len(r_user), dtype=f64, device=dev)
    lnM = float(np.log(float(number_of_items)))
    cl_of_rating = cl_u[ux]
    for c in torch.unique(r_cl).tolist():
        members = torch.nonzero(cl_u == c).ravel()
        Uc = len(members)
        loc = torch.full((U,), -1, dtype=torch.long, device=dev)
        loc[members] = torch.arange(Uc, device=dev)
        m = cl_of_rating == c
        cu, ci, cx = loc[ux[m]], ix[m], x[m]
        bt = w * torch.zeros(I, dtype=f64, device=dev).index_add_(0, ci, beta[ux[m]] * cx)
        S2 = float((beta[members] ** 2).sum())
        XT = torch.sparse_coo_tensor(torch.stack([ci, cu]), cx, size=(I, Uc)).coalesce()
        rsel = torch.nonzero(r_cl == c).ravel()
        cols, col_of_row = torch.unique(r_ix[rsel], return_inverse=True)
        n_row = n_u[r_ux[rsel]]
        for c0 in range(0, len(cols), col_chunk):
            cc = cols[c0:c0 + col_chunk]
            wd = len(cc)
            colpos = torch.full((I,), -1, dtype=torch.long, device=dev)
            colpos[cc] = torch.arange(wd, device=dev)
            inchunk = colpos[ci] >= 0
            Xd = torch.zeros(Uc, wd, dtype=f64, device=dev)
            Xd[cu[inchunk], colpos[ci[inchunk]]] = cx[inchunk]
            G = torch.sparse.mm(XT, Xd)                                             # I x wd
            del Xd
            rr = torch.nonzero((col_of_row >= c0) & (col_of_row < c0 + wd)).ravel()
            if len(rr) == 0:
                continue
            cum = torch.cumsum(n_row[rr], 0)
            a = 0
            while a < len(rr):
                base = int(cum[a - 1]) if a else 0
                z = int(torch.searchsorted(cum, torch.tensor(base + elem_budget, device=dev), right=True))
                z = max(z, a + 1)
                part = rr[a:z]
                g_rows = rsel[part]
                uu_ = r_ux[g_rows]
                cnt = n_row[part]
                rep = torch.repeat_interleave(torch.arange(len(part), device=dev), cnt)
                starts = torch.cumsum(cnt, 0) - cnt
                off = torch.arange(len(rep), device=dev) - starts[rep]
                e_pos = rowptr[uu_][rep] + off
                j = csr_i[e_pos]
                xj = csr_x[e_pos]
                bu = beta[uu_][rep]
                icol = r_ix[g_rows][rep]
                g = G[j, (col_of_row[part] - c0)[rep]]
                e = torch.clamp(bt[j] - w * bu * xj, min=0.0) + p[j] * torch.clamp(S2 - bu * bu, min=0.0)
                term = w * w * g + p[j] * bt[icol] + p[icol] * e
                logsum = torch.zeros(len(part), dtype=f64, device=dev).index_add_(0, rep, torch.log(term))
                nn = cnt.to(f64)
                ref[g_rows] = (nn - 1) * lnM - nn * float(np.log(float(Uc))) + logsum
                a = z
            del G
        del XT
    return ref.cpu().numpy()
