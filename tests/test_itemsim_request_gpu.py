"""Item similarity on request (fy_itemsim_prepare / fy_itemsim_rows): the rows of named items of a prepared job.

Yardstick: the fp64 statement tests/itemsim_measures_ref.py, through its check_rows(..., only_items=...) with its own RTOL = 2e-6,
atol_of and the 5 % cap on boundary pairs (PARITY UNPINNED against the reference: see that file's header).  Where the dot
products are exact on both sides (half stars, integers; every measure but Pearson) the request's rows are also compared BITWISE
with the full build (RowSimilarityJob.run), whose code the request path does not touch.
Thresholds: the five of tests/test_itemsim_measures_gpu.py, cosine 0.2, co-occurrence 2.5 (an integer threshold would put every
pair with that count on the decision boundary)."""
import numpy as np
import pytest

import itemsim_measures_ref as MR
from util import pkg, synth

pytestmark = pytest.mark.gpu
THRESHOLD = {MR.COSINE: 0.2, MR.COOCCURRENCE: 2.5, MR.TANIMOTO: 0.1, MR.LOGLIKELIHOOD: 0.9, MR.CITY_BLOCK: 0.01, MR.EUCLIDEAN: 0.05,
             MR.PEARSON: 0.1}
OPTIONS = [dict(K=30, exclude_self=True, threshold=False), dict(K=100, exclude_self=False, threshold=True)]
EXACT = [m for m in MR.MEASURES if m != MR.PEARSON]      # the measures whose rows are bitwise the full build's on exact data
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
_DATA = {}


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


def data(shape, rm_golden=None):
    if shape not in _DATA:
        if shape == "golden":
            u, i, s = rm_golden["coo"]
            keep = s > 0
            _DATA[shape] = (u[keep], i[keep], s[keep])
        else:
            u, i, s, _ = synth().generate(shape)
            _DATA[shape] = (u.numpy(), i.numpy(), s.numpy())
    return _DATA[shape]


def request_ids(item, seed, share=0.3):
    """-> (ids to ask for, the known ones among them): about `share` of the items, shuffled, a tenth listed twice, plus ids that
    must be passed over -- 0, -5, max + 1, INT32_MIN, INT32_MAX and an id in a hole of the item ids if there is one"""
    rng = np.random.default_rng(seed)
    iid = np.unique(item)
    known = rng.choice(iid, size=max(1, int(share * len(iid))), replace=False)
    stray = [0, -5, int(iid.max()) + 1, INT32_MIN, INT32_MAX]
    holes = np.setdiff1d(np.arange(iid.min(), iid.max() + 1), iid)
    if len(holes):
        stray.append(int(holes[0]))
    assert not set(stray) & set(iid.tolist())
    ids = np.concatenate([known, known[:max(1, len(known) // 10)], np.asarray(stray, dtype=np.int64)])
    rng.shuffle(ids)
    return ids.astype(np.int32), np.sort(known).astype(np.int32)


def walk_of(user, item, known, min_prefs=1):
    """sum over the known items j of sum over the raters v of j of n_v, after the input preparation"""
    deg = np.bincount(user)
    ok = deg[user] >= min_prefs
    user, item = user[ok], item[ok]
    deg = np.bincount(user, minlength=int(user.max()) + 1)
    return int(deg[user[np.isin(item, known)]].astype(np.int64).sum())


def kwargs_of(measure, opt):
    return dict(similarityClassname=measure, maxSimilaritiesPerRow=opt["K"], excludeSelfSimilarity=opt["exclude_self"],
                threshold=THRESHOLD[measure] if opt["threshold"] else None)


def check_request(res, u, i, s, measure, opt, ids, known, min_prefs=1):
    rows, rq = res.rows(), res.request_stats
    thr = THRESHOLD[measure] if opt["threshold"] else None
    info = MR.check_rows(rows, u, i, s, measure, opt["K"], exclude_self=opt["exclude_self"], threshold=thr, min_prefs_per_user=min_prefs,
                         only_items=known)
    print(measure, opt, info, "emitted", len(rows["item"]), rq)
    assert res.stats["recs"] == len(rows["item"]) == res.size
    assert rq["items_asked"] == len(ids) and rq["items_known"] == len(known)
    assert rq["rows_emitted"] == len(np.unique(rows["item"])) == info["rows"]
    assert rq["pair_contribs"] == res.stats["pair_contribs"] == walk_of(u, i, known, min_prefs)
    return info


def same_bits(a, b):
    return (np.array_equal(a["item"], b["item"]) and np.array_equal(a["other"], b["other"])
            and np.array_equal(a["sim"].view(np.uint32), b["sim"].view(np.uint32)))


def rows_of(full, ids):
    """the full build's rows of the listed items, in its order"""
    m = np.isin(full["item"], ids)
    return {k: full[k][m] for k in ("item", "other", "sim")}


# ------------------------------------------------------------------------------------------------ 1. the statement
@pytest.mark.parametrize("shape", ["golden", "tiny", "ml100k"])
@pytest.mark.parametrize("measure", MR.MEASURES)
def test_rows_against_the_statement(ctx, rm_golden, measure, shape):
    u, i, s = data(shape, rm_golden)
    ids, known = request_ids(i, seed=11)
    for opt in OPTIONS:
        job = pkg().RowSimilarityJob(ctx).prepare((u, i, s), **kwargs_of(measure, opt))
        try:
            res = job.rows(ids)
            info = check_request(res, u, i, s, measure, opt, ids, known)
            assert info["rows"] > 0
            assert res.stats["n_users"] == len(np.unique(u)) and res.stats["n_items"] == len(np.unique(i)) and res.stats["nnz"] == len(u)
            assert res.stats["cooc_launches"] == res.request_stats["batches"] == 1 and res.stats["ms_prepare"] == 0
        finally:
            job.close()


# ------------------------------------------------------------------------------------------------ 2. bitwise against the full build
@pytest.mark.parametrize("shape", ["tiny", "ml100k"])
@pytest.mark.parametrize("measure", EXACT)
def test_rows_are_bitwise_the_full_build(ctx, measure, shape):
    u, i, s = data(shape)
    P = pkg()
    for opt in OPTIONS:
        kw = kwargs_of(measure, opt)
        full = P.RowSimilarityJob(ctx).run((u, i, s), **kw).rows()
        job = P.RowSimilarityJob(ctx).prepare((u, i, s), **kw)
        try:
            everything = job.rows(np.unique(i)).rows()
            assert len(full["item"]) > 0 and same_bits(everything, full), (measure, opt)
            ids, known = request_ids(i, seed=5, share=0.2)
            some = job.rows(ids).rows()
            assert same_bits(some, rows_of(full, known)), (measure, opt)
        finally:
            job.close()


# ------------------------------------------------------------------------------------------------ 3. forced shapes
@pytest.mark.parametrize("measure", [MR.LOGLIKELIHOOD, MR.EUCLIDEAN])
def test_forced_chunks_and_batches_give_the_same_bits(ctx, monkeypatch, measure):
    u, i, s = data("ml100k")
    ids, known = request_ids(i, seed=3, share=0.301)      # 506 rows: not a multiple of three
    P = pkg()
    kw = kwargs_of(measure, OPTIONS[0])
    job = P.RowSimilarityJob(ctx).prepare((u, i, s), **kw)
    base = job.rows(ids)
    job.close()
    assert base.request_stats["chunks"] == 1 and base.request_stats["batches"] == 1
    monkeypatch.setenv("FY_ISIM_REQ_CHUNK", "256")      # seven column chunks per row: the merge of the chunks' lists
    job = P.RowSimilarityJob(ctx).prepare((u, i, s), **kw)
    a = job.rows(ids)
    assert a.request_stats["chunks"] == 7 and a.request_stats["batches"] == 1
    assert same_bits(a.rows(), base.rows())
    monkeypatch.setenv("FY_ISIM_REQ_ROWS", "3")         # many batches, the last one short
    b = job.rows(ids)
    job.close()
    assert len(known) % 3 != 0 and b.request_stats["batches"] == -(-len(known) // 3) == b.stats["cooc_launches"]
    assert b.request_stats["chunks"] == 7
    assert same_bits(b.rows(), base.rows())


# ------------------------------------------------------------------------------------------------ 4. list length
def test_list_lengths(ctx):
    u, i, s = data("tiny")
    ids, known = request_ids(i, seed=7)
    P = pkg()
    for K in (1, 1024):      # 1024: more than the 299 items -- whole rows
        opt = dict(K=K, exclude_self=True, threshold=False)
        job = P.RowSimilarityJob(ctx).prepare((u, i, s), **kwargs_of(MR.COSINE, opt))
        res = job.rows(ids)
        job.close()
        check_request(res, u, i, s, MR.COSINE, opt, ids, known)
        per_item = np.bincount(res.rows()["item"])
        assert per_item.max() == 1 if K == 1 else per_item.max() > 100      # (a popular item is co-rated with most of the 299)
    with pytest.raises(RuntimeError, match=r"RowSimilarityJob failed!.*maxSimilaritiesPerRow 1025 exceeds the kernel limit 1024"):
        P.RowSimilarityJob(ctx).prepare((u, i, s), maxSimilaritiesPerRow=1025)
    opt = OPTIONS[0]      # the context is still usable
    job = P.RowSimilarityJob(ctx).prepare((u, i, s), **kwargs_of(MR.TANIMOTO, opt))
    check_request(job.rows(ids), u, i, s, MR.TANIMOTO, opt, ids, known)
    job.close()


# ------------------------------------------------------------------------------------------------ 5. not fp16-exact
@pytest.mark.parametrize("measure", [MR.COSINE, MR.PEARSON])
def test_preferences_that_are_not_fp16_exact(ctx, measure):
    u, i, s = data("tiny")
    s = (s + np.float32(0.1)).astype(np.float32)
    ids, known = request_ids(i, seed=13)
    for opt in OPTIONS:
        job = pkg().RowSimilarityJob(ctx).prepare((u, i, s), **kwargs_of(measure, opt))
        a, b = job.rows(ids), job.rows(ids)
        job.close()
        check_request(a, u, i, s, measure, opt, ids, known)
        assert len(a.rows()["item"]) > 0 and same_bits(a.rows(), b.rows())


# ------------------------------------------------------------------------------------------------ 6. a constant item
def test_pearson_constant_item_has_no_row_and_is_in_no_row(ctx):
    u, i, s = data("tiny")
    s = s.copy()
    cnt = np.bincount(i)
    X = int(np.flatnonzero(cnt >= 5)[0])      # an item with several raters: all of them say 3.0
    s[i == X] = 3.0
    ids, known = request_ids(i, seed=17)
    if X not in known:
        ids, known = np.append(ids, np.int32(X)), np.sort(np.append(known, np.int32(X)))
    opt = OPTIONS[0]
    job = pkg().RowSimilarityJob(ctx).prepare((u, i, s), **kwargs_of(MR.PEARSON, opt))
    res = job.rows(ids)
    job.close()
    check_request(res, u, i, s, MR.PEARSON, opt, ids, known)
    rows = res.rows()
    assert len(rows["item"]) > 0 and X not in rows["item"] and X not in rows["other"]


# ------------------------------------------------------------------------------------------------ 7. input preparation
def test_input_preparation(ctx):
    """ML-100K shape plus one light user who alone rated item 1700: with minPrefsPerUser = 60 that item is lost to the preparation"""
    u, i, s = data("ml100k")
    u = np.concatenate([u, np.array([944, 944, 944], dtype=np.int32)])
    i = np.concatenate([i, np.array([1, 2, 1700], dtype=np.int32)])
    s = np.concatenate([s, np.array([4.0, 3.0, 5.0], dtype=np.float32)])
    deg = np.bincount(u)
    kept_items = np.unique(i[deg[u] >= 60])
    ids, known = request_ids(i, seed=19)
    ids = np.append(ids, np.int32(1700))
    known = np.intersect1d(known, kept_items).astype(np.int32)
    assert 1700 not in kept_items and 1700 not in known
    opt = dict(K=25, exclude_self=True, threshold=False)
    job = pkg().RowSimilarityJob(ctx).prepare((u, i, s), minPrefsPerUser=60, **kwargs_of(MR.LOGLIKELIHOOD, opt))
    res = job.rows(ids)
    job.close()
    check_request(res, u, i, s, MR.LOGLIKELIHOOD, opt, ids, known, min_prefs=60)
    assert res.stats["n_users"] == int((deg >= 60).sum()) < int((deg > 0).sum())
    assert 1700 not in res.rows()["item"] and 1700 not in res.rows()["other"]


# ------------------------------------------------------------------------------------------------ 8. reuse
def test_one_job_answers_many_requests(ctx):
    u, i, s = data("tiny")
    P = pkg()
    r = P.Ratings(ctx, u, i, s)
    opt = OPTIONS[0]
    job = P.RowSimilarityJob(ctx).prepare(r, **kwargs_of(MR.LOGLIKELIHOOD, opt))
    r.close()      # the job owns what it needs
    asked = [request_ids(i, seed=k) for k in (1, 2, 3)]
    answers = [job.rows(ids) for ids, _ in asked]
    for (ids, known), res in zip(asked, answers):
        check_request(res, u, i, s, MR.LOGLIKELIHOOD, opt, ids, known)
    assert not same_bits(answers[0].rows(), answers[1].rows())
    assert same_bits(job.rows(asked[0][0]).rows(), answers[0].rows())
    empty = job.rows(np.zeros(0, dtype=np.int32))
    assert empty.size == 0 and len(empty.rows()["item"]) == 0
    assert empty.request_stats["items_asked"] == 0 and empty.request_stats["items_known"] == 0 and empty.request_stats["batches"] == 0
    assert same_bits(job.rows(asked[0][0]).rows(), answers[0].rows())
    job.close()


def test_a_job_over_no_preferences_answers_with_nothing(ctx):
    z = np.zeros(0, dtype=np.int32)
    job = pkg().RowSimilarityJob(ctx).prepare((z, z, np.zeros(0, dtype=np.float32)))
    res = job.rows([1, 2, 3])
    assert res.size == 0 and res.request_stats["items_asked"] == 3 and res.request_stats["items_known"] == 0
    job.close()


# ------------------------------------------------------------------------------------------------ 9. item-row shards
def test_item_row_shards_partition_a_request(ctx):
    u, i, s = data("tiny")
    P = pkg()
    ids, known = request_ids(i, seed=23)
    kw = dict(similarityClassname=MR.TANIMOTO, maxSimilaritiesPerRow=10)
    job = P.RowSimilarityJob(ctx).prepare((u, i, s), **kw)
    whole = job.rows(ids).rows()
    job.close()
    parts = []
    for rank in range(3):
        job = P.RowSimilarityJob(ctx).prepare((u, i, s), rank=rank, world=3, **kw)
        parts.append(job.rows(ids).rows())
        job.close()
        shard = np.unique(P.RowSimilarityJob(ctx).run((u, i, s), rank=rank, world=3, **kw).rows()["item"])
        assert len(parts[-1]["item"]) > 0 and np.all(np.isin(parts[-1]["item"], shard))
    items = [set(p["item"].tolist()) for p in parts]
    assert not (items[0] & items[1]) and not (items[0] & items[2]) and not (items[1] & items[2])
    key = lambda rows: sorted(zip(rows["item"].tolist(), rows["other"].tolist(), rows["sim"].view(np.uint32).tolist()))
    merged = {k: np.concatenate([p[k] for p in parts]) for k in ("item", "other", "sim")}
    assert key(merged) == key(whole)
    MR.check_rows(whole, u, i, s, MR.TANIMOTO, 10, only_items=known)


# ------------------------------------------------------------------------------------------------ 10. after a write
def test_after_a_write_prepare_again(ctx):
    u, i, s = data("tiny")
    P = pkg()
    cnt = np.bincount(i)
    X = int(np.argmax(cnt))
    raters = u[i == X]
    stranger = int(np.setdiff1d(np.unique(u), raters)[0])
    opt = OPTIONS[0]
    kw = kwargs_of(MR.COSINE, opt)
    r = P.Ratings(ctx, u, i, s)
    old_job = P.RowSimilarityJob(ctx).prepare(r, **kw)
    before = old_job.rows([X]).rows()
    # one upsert to an existing key, one insert, one delete, all touching item X
    r2 = r.updated(np.array([raters[0], stranger, raters[1]], dtype=np.int32), np.array([X, X, X], dtype=np.int32),
                   np.array([0.5, 5.0, 0.0], dtype=np.float32), remove=np.array([0, 0, 1], dtype=np.uint8))
    assert r2.update_stats["n_replaced"] == 1 and r2.update_stats["n_inserted"] == 1 and r2.update_stats["n_deleted"] == 1
    u2, i2, s2 = r2.to_host()
    new_job = P.RowSimilarityJob(ctx).prepare(r2, **kw)
    r.close()
    r2.close()
    ids, known = np.array([X], dtype=np.int32), np.array([X], dtype=np.int32)
    res = new_job.rows(ids)
    check_request(res, u2, i2, s2, MR.COSINE, opt, ids, known)
    assert not same_bits(res.rows(), before)
    assert same_bits(old_job.rows([X]).rows(), before)      # the job prepared earlier still answers for the old ratings
    MR.check_rows(before, u, i, s, MR.COSINE, opt["K"], only_items=known)
    old_job.close()
    new_job.close()


# ------------------------------------------------------------------------------------------------ 11. unsupported configurations
def test_unsupported_configurations_fail_at_prepare_and_leave_the_context_usable(ctx):
    u, i, s = data("tiny")
    job = pkg().RowSimilarityJob(ctx)
    with pytest.raises(RuntimeError, match=r"RowSimilarityJob failed!.*SIMILARITY_PEARSON_CORRELATION with a threshold <= 0"):
        job.prepare((u, i, s), similarityClassname=MR.PEARSON, threshold=-0.5)
    neg = s.copy()
    neg[5] = -1.0
    with pytest.raises(RuntimeError, match=r"RowSimilarityJob failed!.*SIMILARITY_EUCLIDEAN_DISTANCE on data with a non-positive preference"):
        job.prepare((u, i, neg), similarityClassname=MR.EUCLIDEAN)
    ids, known = request_ids(i, seed=11)
    for opt in OPTIONS:
        prepared = job.prepare((u, i, s), **kwargs_of(MR.COSINE, opt))
        info = check_request(prepared.rows(ids), u, i, s, MR.COSINE, opt, ids, known)
        prepared.close()
        assert info["rows"] > 0


def test_preferences_that_are_not_positive(ctx):
    """signed contributions add modulo 2^64 and read back signed: cosine on preferences shifted below zero"""
    u, i, s = data("tiny")
    s = (s - np.float32(2.5)).astype(np.float32)      # -2 .. 2.5 in half steps, zeros included
    ids, known = request_ids(i, seed=29)
    opt = dict(K=30, exclude_self=True, threshold=True)
    job = pkg().RowSimilarityJob(ctx).prepare((u, i, s), **kwargs_of(MR.COSINE, opt))
    res = job.rows(ids)
    job.close()
    check_request(res, u, i, s, MR.COSINE, opt, ids, known)
    assert len(res.rows()["item"]) > 0


# ------------------------------------------------------------------------------------------------ 12. itemsFile
def test_items_file(ctx, tmp_path):
    u, i, s = data("tiny")
    P = pkg()
    ids, known = request_ids(i, seed=31)
    path = tmp_path / "items.txt"
    path.write_text("\n".join(str(int(x)) for x in ids) + "\nnot an id\n")
    kw = kwargs_of(MR.CITY_BLOCK, OPTIONS[0])
    a = P.RowSimilarityJob(ctx).run((u, i, s), itemsFile=str(path), **kw)
    job = P.RowSimilarityJob(ctx).prepare((u, i, s), **kw)
    b = job.rows(P.read_id_file(str(path)))
    job.close()
    assert a.request_stats["items_known"] == len(known) == b.request_stats["items_known"]
    assert len(a.rows()["item"]) > 0 and same_bits(a.rows(), b.rows())
    c = P.RowSimilarityJob(ctx).run((u, i, s), itemsFile=ids, **kw)      # an array instead of a path
    assert same_bits(c.rows(), a.rows())
    assert P.RowSimilarityJob(ctx).run((u, i, s), **kw).request_stats is None      # the full build's result has none


def test_ids_outside_int32_are_passed_over_not_wrapped(ctx):
    u, i, s = data("tiny")
    P = pkg()
    job = P.RowSimilarityJob(ctx).prepare((u, i, s), maxSimilaritiesPerRow=5)
    a = job.rows(np.array([5, 7], dtype=np.int64))
    b = job.rows(np.array([2 ** 32 + 5, 7, -2 ** 32 + 9, 2 ** 40], dtype=np.int64))      # 2^32 + 5 is not item 5
    job.close()
    assert np.unique(a.rows()["item"]).tolist() == [5, 7] and a.request_stats["items_known"] == 2
    assert np.unique(b.rows()["item"]).tolist() == [7] and b.request_stats["items_known"] == 1
    c = P.RowSimilarityJob(ctx).run((u, i, s), maxSimilaritiesPerRow=5, itemsFile=np.array([2 ** 32 + 5, 7], dtype=np.int64))
    assert same_bits(c.rows(), b.rows())


def test_a_full_build_leaves_no_error_message(ctx):
    u, i, s = data("tiny")
    P = pkg()
    lib = P._native.load()
    with pytest.raises(RuntimeError):
        P.RowSimilarityJob(ctx).prepare((u, i, s), maxSimilaritiesPerRow=0)
    before = lib.fy_last_error()
    res = P.RowSimilarityJob(ctx).run((u, i, s), maxSimilaritiesPerRow=5)
    assert res.request_stats is None and lib.fy_last_error() == before and b"fy_itemsim_rows" not in lib.fy_last_error()
