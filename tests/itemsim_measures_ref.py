"""The seven RowSimilarityJob measures as an fp64 statement (numpy, dense B^T B: small shapes only) -- the yardstick of
tests/test_itemsim_measures_*.py.

PARITY UNPINNED against the reference, exactly as oracle/itemsim_oracle.c says for cosine: Mahout's `measures` package is not in
the reference tree, no jar of it exists on the build machine and the reference has no fixture for this path.  The formulas below
are restated from Mahout 0.8's published classes (CountbasedMeasure, TanimotoCoefficientSimilarity, LoglikelihoodSimilarity +
stats.LogLikelihood, CityBlockSimilarity, EuclideanDistanceSimilarity, PearsonCorrelationSimilarity); they are the contract the
library implements (include/filmyou.h), not a recording of a Mahout run.

After the input preparation (users with fewer than min_prefs_per_user preferences dropped), let r_ui be the kept preferences,
n_i the number of users with a preference for item i, N the number of distinct users that still have a preference, and for a
pair (i, j) that at least one user co-rated, d = sum_u w_ui w_uj:

  name                              column transform w_ui                              norm a_i       similarity
  SIMILARITY_COSINE                 r_ui / ||r_.i||_2                                  -              d
  SIMILARITY_COOCCURRENCE           1                                                  -              d
  SIMILARITY_TANIMOTO_COEFFICIENT   1                                                  n_i            d / (a_i + a_j - d)
  SIMILARITY_LOGLIKELIHOOD          1                                                  n_i            1 - 1 / (1 + LLR(k11 = d, k12 = a_j - d,
                                                                                                      k21 = a_i - d, k22 = N - a_i - a_j + d))
  SIMILARITY_CITY_BLOCK             1                                                  n_i            1 / (1 + a_i + a_j - 2 d)
  SIMILARITY_EUCLIDEAN_DISTANCE     r_ui                                               sum_u r_ui^2   1 / (1 + sqrt(max(0, a_i - 2 d + a_j)))
  SIMILARITY_PEARSON_CORRELATION    c_ui / ||c_.i||_2, c_ui = r_ui - (sum_u |r_ui|) / n_i   -         d

LLR(k11, k12, k21, k22) = 0 if rowE + colE < matE, else 2 (rowE + colE - matE), H(x...) = xlogx(sum x) - sum xlogx(x),
xlogx(0) = 0, xlogx(x) = x ln x, rowE = H(k11 + k12, k21 + k22), colE = H(k11 + k21, k12 + k22), matE = H(k11, k12, k21, k22).

Kept: j != i when exclude_self, sim >= threshold (no threshold: sim > 0); NaN (Pearson of a constant item) is dropped; best first,
ties by ascending item id.  Mahout's consider() pre-pruning and random down-sampling are not modelled.
"""
import numpy as np

COSINE, COOCCURRENCE, TANIMOTO, LOGLIKELIHOOD, CITY_BLOCK, EUCLIDEAN, PEARSON = (
    "SIMILARITY_COSINE", "SIMILARITY_COOCCURRENCE", "SIMILARITY_TANIMOTO_COEFFICIENT", "SIMILARITY_LOGLIKELIHOOD",
    "SIMILARITY_CITY_BLOCK", "SIMILARITY_EUCLIDEAN_DISTANCE", "SIMILARITY_PEARSON_CORRELATION")
MEASURES = (COSINE, COOCCURRENCE, TANIMOTO, LOGLIKELIHOOD, CITY_BLOCK, EUCLIDEAN, PEARSON)


def xlogx(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0.0, 0.0, x * np.log(x))


def entropy(*xs):
    return xlogx(sum(xs)) - sum(xlogx(x) for x in xs)


def llr(k11, k12, k21, k22):
    row_e = entropy(k11 + k12, k21 + k22)
    col_e = entropy(k11 + k21, k12 + k22)
    mat_e = entropy(k11, k12, k21, k22)
    return np.where(row_e + col_e < mat_e, 0.0, 2.0 * (row_e + col_e - mat_e))


def prepare(user, item, score, min_prefs_per_user=1):
    """-> (R [users x items] fp64, B the same as 0 / 1, raw item ids of the columns); users below min_prefs_per_user dropped"""
    user, item = np.asarray(user).astype(np.int64), np.asarray(item).astype(np.int64)
    score = np.asarray(score, dtype=np.float64)
    ok = ~np.isnan(score)
    user, item, score = user[ok], item[ok], score[ok]
    uid, du = np.unique(user, return_inverse=True)
    deg = np.bincount(du, minlength=len(uid))
    ok = deg[du] >= min_prefs_per_user
    user, item, score = user[ok], item[ok], score[ok]
    uid, du = np.unique(user, return_inverse=True)
    iid, di = np.unique(item, return_inverse=True)
    R = np.zeros((len(uid), len(iid)))
    B = np.zeros((len(uid), len(iid)))
    R[du, di] = score
    B[du, di] = 1.0
    return R, B, iid


def similarity_matrix(user, item, score, measure, min_prefs_per_user=1):
    """-> (S [items x items] fp64 similarity of every pair, co-rated [items x items] bool, raw item ids, N)"""
    R, B, iid = prepare(user, item, score, min_prefs_per_user)
    N = float(R.shape[0])
    C = B.T @ B                       # users who rated both: exact integers
    corated = C > 0
    n = B.sum(axis=0)
    ai, aj = n[:, None], n[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        if measure == COSINE:
            S = (R / np.sqrt((R * R).sum(axis=0))).T @ (R / np.sqrt((R * R).sum(axis=0)))
        elif measure == COOCCURRENCE:
            S = C
        elif measure == TANIMOTO:
            S = C / (ai + aj - C)
        elif measure == LOGLIKELIHOOD:
            S = 1.0 - 1.0 / (1.0 + llr(C, aj - C, ai - C, N - ai - aj + C))
        elif measure == CITY_BLOCK:
            S = 1.0 / (1.0 + ai + aj - 2.0 * C)
        elif measure == EUCLIDEAN:
            a = (R * R).sum(axis=0)
            S = 1.0 / (1.0 + np.sqrt(np.maximum(0.0, a[:, None] - 2.0 * (R.T @ R) + a[None, :])))
        elif measure == PEARSON:
            centre = np.abs(R).sum(axis=0) / n
            Cn = (R - centre[None, :]) * B
            W = np.where(B > 0, Cn / np.sqrt((Cn * Cn).sum(axis=0))[None, :], 0.0)      # 0 / 0 = NaN on a constant item's raters
            S = np.nan_to_num(W, nan=0.0).T @ np.nan_to_num(W, nan=0.0)
            const = np.isnan(W).any(axis=0)
            S[const, :] = np.nan
            S[:, const] = np.nan
        else:
            raise ValueError(measure)
    return S, corated, iid, N


def itemsim(user, item, score, measure, max_similarities_per_item=1 << 30, exclude_self=True, threshold=None, min_prefs_per_user=1):
    """The job's result: {"item", "other", "sim" (fp64)} grouped by item, best first, ties by ascending item id, plus
    "corated": the number of ordered pairs (after exclude_self) that at least one user co-rated and "n_users": N."""
    S, corated, iid, N = similarity_matrix(user, item, score, measure, min_prefs_per_user)
    if exclude_self:
        corated = corated & ~np.eye(len(iid), dtype=bool)
    with np.errstate(invalid="ignore"):
        keep = corated & ((S >= threshold) if threshold is not None else (S > 0.0))      # NaN fails both
    items, others, sims = [], [], []
    for a in range(len(iid)):
        cols = np.flatnonzero(keep[a])
        cols = cols[np.lexsort((iid[cols], -S[a, cols]))][:max_similarities_per_item]
        items.append(np.full(len(cols), iid[a]))
        others.append(iid[cols])
        sims.append(S[a, cols])
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
    return {"item": cat(items, np.int32), "other": cat(others, np.int32), "sim": cat(sims, np.float64), "corated": int(corated.sum()),
            "n_users": int(N)}


# ---------------------------------------------------------------------------------------------------------------- comparison
RTOL = 2e-6            # the project's bound for an emitted float32 similarity against fp64 (tests/test_itemsim_gpu.py)
OPTIONAL_CAP = 0.05    # at most this share of an input's co-rated pairs may sit on the decision boundary


def atol_of(measure, n_users, fp64_weights=False):
    """The absolute term on top of RTOL, derived per measure (not tuned):
    - Tanimoto, city block, Euclidean distance, co-occurrence: 0 -- integer or fp16-exact dot products, exact in fp64, and the same
      fp64 operations on both sides;
    - log-likelihood: 64 * 2^-52 * N ln N -- about ten x ln x terms of size <= N ln N, a few ulp each, and |d sim / d LLR| <= 1
      (9e-11 at 943 users);
    - Pearson: the library's weights are fp32, each off by <= 2^-24 relative, and sum |w_i w_j| <= 1 by Cauchy-Schwarz, so
      |delta d| <= 2^-23; doubled for margin: 2^-22.  (With fp64 weights it would be 64 * 2^-52.)
    - cosine: 0, as in tests/test_itemsim_gpu.py."""
    if measure == LOGLIKELIHOOD:
        return 64.0 * 2.0 ** -52 * n_users * np.log(max(n_users, 2))
    if measure == PEARSON:
        return 64.0 * 2.0 ** -52 if fp64_weights else 2.0 ** -22
    return 0.0


def check_rows(rows, user, item, score, measure, K, exclude_self=True, threshold=None, min_prefs_per_user=1, only_items=None):
    """Compares emitted rows {"item", "other", "sim"} with the statement, tolerant of the decision boundary within a stated cap.

    Membership is a strict comparison (sim > 0, sim >= threshold) and some reference values sit on it exactly (independent counts:
    LLR = 0; centred products that cancel: Pearson 0).  A co-rated reference pair with |sim - bound| <= atol + RTOL |bound| (bound =
    0 or the threshold) is OPTIONAL; every other co-rated pair that passes the bound is FIRM.  Per item: the row's length lies
    between min(K, firm) and min(K, firm + optional); every emitted pair is a firm or optional pair of the reference with a
    matching value, no duplicates, no self pair when excluded; values non-increasing, exact ties (equal emitted floats whose reference
    values are equal too) in ascending item id; the k-th emitted value is not worse than the
    k-th best firm value (nothing better was left out) and not better than the k-th best of firm + optional.  Optional pairs may be
    at most OPTIONAL_CAP of the input's co-rated pairs.  Returns counts for the test to print.
    only_items: the raw item ids whose rows `rows` holds (an item-row shard); default every item."""
    S, corated, iid, N = similarity_matrix(user, item, score, measure, min_prefs_per_user)
    atol = atol_of(measure, N)
    if exclude_self:
        corated = corated & ~np.eye(len(iid), dtype=bool)
    bound = 0.0 if threshold is None else float(threshold)
    slack = atol + RTOL * abs(bound)
    with np.errstate(invalid="ignore"):
        valid = corated & ~np.isnan(S)
        optional = valid & (np.abs(S - bound) <= slack)
        firm = valid & ~optional & ((S >= bound) if threshold is not None else (S > 0.0))
    n_corated = int(corated.sum())
    assert int(optional.sum()) <= OPTIONAL_CAP * max(n_corated, 1), (int(optional.sum()), n_corated)
    col_of = {int(x): k for k, x in enumerate(iid)}
    got = {}
    for a, b, s in zip(rows["item"], rows["other"], rows["sim"]):
        got.setdefault(int(a), []).append((int(b), float(s)))
    mine = set(col_of) if only_items is None else {int(x) for x in only_items}
    must = {int(iid[a]) for a in range(len(iid)) if firm[a].any()} & mine
    may = {int(iid[a]) for a in range(len(iid)) if (firm[a] | optional[a]).any()} & mine
    assert must <= set(got) <= may, (sorted(must - set(got))[:5], sorted(set(got) - may)[:5])
    lenient = 0
    for a_raw, lst in got.items():
        a = col_of[a_raw]
        nf, no = int(firm[a].sum()), int(optional[a].sum())
        assert min(K, nf) <= len(lst) <= min(K, nf + no), (a_raw, len(lst), nf, no)
        cols = np.array([col_of[b] for b, _ in lst])
        sims = np.array([s for _, s in lst])
        assert len(set(cols.tolist())) == len(cols) and (not exclude_self or np.all(cols != a))
        assert np.all(firm[a, cols] | optional[a, cols]), (a_raw, "a pair the reference does not keep")
        want = S[a, cols]
        assert np.all(np.abs(sims - want) <= RTOL * np.abs(want) + atol), (a_raw, float(np.abs(sims - want).max()))
        assert np.all(sims[:-1] >= sims[1:])
        tied = (sims[:-1] == sims[1:]) & (want[:-1] == want[1:])      # exactly equal in the reference too: ascending item id
        assert np.all(iid[cols[:-1]][tied] < iid[cols[1:]][tied]), (a_raw, "ties must come in ascending item id")
        best_firm = np.sort(S[a, firm[a]])[::-1][:len(lst)]
        k = len(best_firm)
        assert np.all(sims[:k] >= best_firm - (RTOL * np.abs(best_firm) + atol)), (a_raw, "something better was left out")
        best_any = np.sort(S[a, firm[a] | optional[a]])[::-1][:len(lst)]
        assert np.all(sims <= best_any + (RTOL * np.abs(best_any) + atol)), (a_raw, "better than the reference's k-th best")
        lenient += int(min(K, nf + no) > min(K, nf))
    return {"corated": n_corated, "optional": int(optional.sum()), "firm": int(firm.sum()), "rows": len(got), "rows_at_the_boundary": lenient}
