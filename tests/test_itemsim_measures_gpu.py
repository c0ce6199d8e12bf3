"""The five RowSimilarityJob measures beside cosine and co-occurrence, on the GPU, against the fp64 statement of
tests/itemsim_measures_ref.py (PARITY UNPINNED against the reference: see that file's header).

Tolerances are derived in itemsim_measures_ref.atol_of (RTOL = 2e-6 of tests/test_itemsim_gpu.py plus a per-measure absolute
term; Pearson's is the fp32-weights one, 2^-22: the library's Pearson weights are fp32).  check_rows tolerates the decision
boundary (a reference value within the tolerance of 0 or of the threshold is optional) and asserts that such entries are at most
5 % of the input's co-rated pairs.  Every figure it returns is printed before the next assertion.

The symmetric build (upper triangle + band sweep) admits Tanimoto, log-likelihood, city block and Euclidean distance when
FY_ISIM_GRAM=1 forces it; Pearson never takes it."""
import numpy as np
import pytest

import itemsim_measures_ref as MR
import oracle
from util import pkg, synth

pytestmark = pytest.mark.gpu
NEW = [MR.TANIMOTO, MR.LOGLIKELIHOOD, MR.CITY_BLOCK, MR.EUCLIDEAN, MR.PEARSON]
# a positive threshold per measure, inside the range its values take on these inputs (chosen before any run; city block and
# Euclidean similarities of items with tens of raters are small)
THRESHOLD = {MR.TANIMOTO: 0.1, MR.LOGLIKELIHOOD: 0.9, MR.CITY_BLOCK: 0.01, MR.EUCLIDEAN: 0.05, MR.PEARSON: 0.1}


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


def data(shape, rm_golden):
    if shape == "golden":
        u, i, s = rm_golden["coo"]
        keep = s > 0
        return u[keep], i[keep], s[keep]
    u, i, s, _ = synth().generate(shape)
    return u.numpy(), i.numpy(), s.numpy()


def run_and_check(ctx, u, i, s, measure, K, exclude_self=True, threshold=None, min_prefs=1, **kw):
    res = pkg().RowSimilarityJob(ctx).run((u, i, s), similarityClassname=measure, maxSimilaritiesPerRow=K, excludeSelfSimilarity=exclude_self,
                                          threshold=threshold, minPrefsPerUser=min_prefs, **kw)
    info = MR.check_rows(res.rows(), u, i, s, measure, K, exclude_self=exclude_self, threshold=threshold, min_prefs_per_user=min_prefs)
    print(measure, "K", K, "threshold", threshold, "exclude_self", exclude_self, info, "emitted", len(res.rows()["item"]))
    assert info["rows"] > 0
    return res, info


@pytest.mark.parametrize("shape", ["golden", "tiny", "ml100k"])
@pytest.mark.parametrize("measure", NEW)
def test_measure(ctx, rm_golden, measure, shape):
    u, i, s = data(shape, rm_golden)
    res, _ = run_and_check(ctx, u, i, s, measure, 30)
    n = np.bincount(u)
    assert res.stats["unordered_pairs"] == int((n.astype(np.int64) * (n - 1) // 2).sum())
    run_and_check(ctx, u, i, s, measure, 100, exclude_self=False, threshold=THRESHOLD[measure])


@pytest.mark.parametrize("measure", [MR.LOGLIKELIHOOD, MR.PEARSON])
def test_ml100k_lists_never_reach_the_boundary(ctx, measure):
    """every ML-100K-shaped row has more than 100 firm candidates for these two: no leniency is used there"""
    u, i, s, _ = synth().generate("ml100k")
    _, info = run_and_check(ctx, u.numpy(), i.numpy(), s.numpy(), measure, 100)
    assert info["rows_at_the_boundary"] == 0


@pytest.mark.parametrize("env", [{"FY_COOC_MAX_CH": "256", "FY_ISIM_HEAVY": "8"},      # column chunks, heavy rows split by chunk + merge
                                 {"FY_COOC_MAX_CH": "256", "FY_ISIM_HEAVY": "1000000"},  # column chunks, threshold carried along
                                 {"FY_COOC_PK": "0"}])                                   # 8-byte CSR entries
@pytest.mark.parametrize("measure", [MR.LOGLIKELIHOOD, MR.EUCLIDEAN])
def test_forced_paths(ctx, monkeypatch, measure, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    u, i, s, _ = synth().generate("ml100k")
    run_and_check(ctx, u.numpy(), i.numpy(), s.numpy(), measure, 30)


def test_loglikelihood_counts_the_users_that_survive(ctx):
    """minPrefsPerUser = 60 drops users: N (the reference's --numberOfColumns) must be the number that is left"""
    u, i, s, _ = synth().generate("ml100k")
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    res, _ = run_and_check(ctx, u, i, s, MR.LOGLIKELIHOOD, 25, min_prefs=60)
    deg = np.bincount(u)
    assert res.stats["n_users"] == int((deg >= 60).sum()) < int((deg > 0).sum())


def test_tanimoto_item_row_shards_partition_the_result(ctx):
    u, i, s, _ = synth().generate("tiny")
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    job = pkg().RowSimilarityJob(ctx)
    whole = job.run((u, i, s), similarityClassname=MR.TANIMOTO, maxSimilaritiesPerRow=10).rows()
    parts = [job.run((u, i, s), similarityClassname=MR.TANIMOTO, maxSimilaritiesPerRow=10, rank=r, world=3).rows() for r in range(3)]
    key = lambda rows: sorted(zip(rows["item"].tolist(), rows["other"].tolist(), rows["sim"].tolist()))
    merged = {k: np.concatenate([p[k] for p in parts]) for k in ("item", "other", "sim")}
    assert key(merged) == key(whole)
    assert len({int(x) for p in parts for x in np.unique(p["item"])}) == len(np.unique(whole["item"]))
    MR.check_rows(whole, u, i, s, MR.TANIMOTO, 10)


SYMMETRIC = [{"FY_ISIM_GRAM": "1"},                                                        # one chunk of the walk, one piece per band
             {"FY_ISIM_GRAM": "1", "FY_COOC_MAX_CH": "256", "FY_ISIM_PIECE": "128"},      # several chunks, several pieces per band
             {"FY_ISIM_GRAM": "1", "FY_ISIM_CAPG": "40"},                                 # candidate lists overflow: rows redone exactly
             {"FY_ISIM_GRAM": "1", "FY_ISIM_ACC32": "0", "FY_COOC_MAX_CH": "512"}]        # 64-bit fixed-point accumulators
# (the variants of tests/test_itemsim_gpu.py::SYMMETRIC)


@pytest.mark.parametrize("env", SYMMETRIC)
@pytest.mark.parametrize("measure", [MR.TANIMOTO, MR.LOGLIKELIHOOD, MR.CITY_BLOCK, MR.EUCLIDEAN])
def test_symmetric_build_forced(ctx, monkeypatch, measure, env):
    """The symmetric build (upper triangle by the RM2 row kernel + band sweep) admits these four; FY_ISIM_GRAM=1 forces it.  Against
    the statement, AND row for row identical (items and float bits) to the row-at-a-time build of the same job: the dot products
    are exact in both and the finish function is shared."""
    u, i, s, _ = synth().generate("ml100k")
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    monkeypatch.setenv("FY_ISIM_GRAM", "0")
    a = pkg().RowSimilarityJob(ctx).run((u, i, s), similarityClassname=measure, maxSimilaritiesPerRow=30)
    assert a.stats["cooc_launches"] == 1 and a.stats["isim_candidates"] == 0
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    b, info = run_and_check(ctx, u, i, s, measure, 30)
    print(measure, env, "candidates", b.stats["isim_candidates"], "redone rows", b.stats["isim_redone_rows"])
    assert b.stats["cooc_launches"] == 1 and b.stats["isim_candidates"] > 0      # the route ran
    ra, rb = a.rows(), b.rows()
    assert np.array_equal(ra["item"], rb["item"]) and np.array_equal(ra["other"], rb["other"])
    assert np.array_equal(ra["sim"].view(np.uint32), rb["sim"].view(np.uint32))


@pytest.mark.parametrize("measure", [MR.TANIMOTO, MR.EUCLIDEAN])
def test_symmetric_build_with_self_similarity_and_threshold(ctx, monkeypatch, measure):
    """the diagonal candidate and the job's own threshold on the symmetric build"""
    monkeypatch.setenv("FY_ISIM_GRAM", "1")
    u, i, s, _ = synth().generate("ml100k")
    res, _ = run_and_check(ctx, u.numpy(), i.numpy(), s.numpy(), measure, 100, exclude_self=False, threshold=THRESHOLD[measure])
    assert res.stats["isim_candidates"] > 0


def test_pearson_never_takes_the_symmetric_build(ctx, monkeypatch):
    monkeypatch.setenv("FY_ISIM_GRAM", "1")
    u, i, s, _ = synth().generate("ml100k")
    res, _ = run_and_check(ctx, u.numpy(), i.numpy(), s.numpy(), MR.PEARSON, 30)
    assert res.stats["cooc_launches"] == 1 and res.stats["isim_candidates"] == 0      # the row-at-a-time route


def test_unsupported_configurations_fail_and_leave_the_context_usable(ctx):
    u, i, s, _ = synth().generate("tiny")
    u, i, s = u.numpy(), i.numpy(), s.numpy().copy()
    job = pkg().RowSimilarityJob(ctx)
    with pytest.raises(RuntimeError, match=r"RowSimilarityJob failed!.*SIMILARITY_PEARSON_CORRELATION with a threshold <= 0"):
        job.run((u, i, s), similarityClassname=MR.PEARSON, threshold=-0.5)
    neg = s.copy()
    neg[5] = -1.0
    with pytest.raises(RuntimeError, match=r"RowSimilarityJob failed!.*SIMILARITY_EUCLIDEAN_DISTANCE on data with a non-positive preference"):
        job.run((u, i, neg), similarityClassname=MR.EUCLIDEAN)
    import test_itemsim_gpu as IS
    res = job.run((u, i, s), maxSimilaritiesPerRow=20)      # a cosine job after them, checked like test_itemsim_gpu.py::test_synthetic
    ref = oracle.itemsim(u, i, s, max_similarities_per_item=1 << 30)
    assert len(res.rows()["item"]) > 0
    IS.check(res.rows(), ref, 20)      # (rows are grouped by item in popularity order, the oracle's in ascending id: compared per item)


@pytest.mark.parametrize("name", ["SIMILARITY_TANIMOTO_COEFFICIENT",
                                  "class org.apache.mahout.math.hadoop.similarity.cooccurrence.measures.LoglikelihoodSimilarity"])
def test_baseline_recommender_job_takes_the_measures(ctx, name):
    """checked like test_itemcf_gpu.py::run_both: the item-CF oracle consumes the GPU's own similarity rows, which are checked
    against the statement here"""
    import test_itemcf_gpu as CF
    u, i, s, _ = synth().generate("tiny")
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    rec, sims = pkg().BaselineRecommenderJob(ctx).run((u, i, s), numRecommendations=10, maxPrefsPerUser=10, maxSimilaritiesPerItem=15,
                                                      similarityClassname=name)
    srows = sims.rows()
    measure = MR.TANIMOTO if "TANIMOTO" in name else MR.LOGLIKELIHOOD
    print(MR.check_rows(srows, u, i, s, measure, 15))
    ref = oracle.itemcf(u, i, s, srows["item"], srows["other"], srows["sim"].astype(np.float64), num_recommendations=1 << 30,
                        max_prefs_per_user=10, boolean_data=False)
    CF.check(rec.rows(), ref, 10)
