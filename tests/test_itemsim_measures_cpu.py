"""Pins the fp64 statement of the seven RowSimilarityJob measures (tests/itemsim_measures_ref.py) -- no GPU.

Hand-computed values on a 4-user x 3-item matrix, the statement's cosine / co-occurrence against the C oracle on the reference's
golden matrix, the comparator the GPU tests use, and the name -> enum mapping of the Python host."""
import math

import numpy as np
import pytest

import itemsim_measures_ref as MR
import oracle
from util import pkg

# users 1..4 (rows) x items 1..3; '.' = no preference
#        i1  i2  i3
#   u1    5   3   .
#   u2    4   .   4
#   u3    .   3   2
#   u4    1   3   .
U = np.array([1, 1, 2, 2, 3, 3, 4, 4], dtype=np.int32)
I = np.array([1, 2, 1, 3, 2, 3, 1, 2], dtype=np.int32)
S = np.array([5, 3, 4, 4, 3, 2, 1, 3], dtype=np.float32)
# n = (3, 3, 2), N = 4; co-rating counts d12 = 2 (u1, u4), d13 = 1 (u2), d23 = 1 (u3)


def pairs(measure, **kw):
    r = MR.itemsim(U, I, S, measure, **kw)
    return {(int(a), int(b)): float(s) for a, b, s in zip(r["item"], r["other"], r["sim"])}


def test_llr_of_the_textbook_table():
    # k = (1, 0, 0, 1): rowE = colE = matE = 2 ln 2, LLR = 2 * 2 ln 2
    assert MR.llr(1, 0, 0, 1) == pytest.approx(4 * math.log(2), rel=1e-15)
    assert 4 * math.log(2) == pytest.approx(2.7726, abs=5e-5)
    assert 1 - 1 / (1 + MR.llr(1, 0, 0, 1)) == pytest.approx(0.73493, abs=5e-6)      # 1 - 1 / 3.772589 = 0.734930
    # independent counts (k11 N = row x column): LLR = 0
    assert float(MR.llr(2, 2, 2, 2)) == pytest.approx(0.0, abs=1e-14)
    assert MR.xlogx(0.0) == 0.0


def test_tanimoto():
    p = pairs(MR.TANIMOTO)
    assert p[(1, 2)] == p[(2, 1)] == 2 / (3 + 3 - 2)
    assert p[(1, 3)] == 1 / (3 + 2 - 1) and p[(2, 3)] == 1 / (3 + 2 - 1)
    q = pairs(MR.TANIMOTO, exclude_self=False)
    assert q[(1, 1)] == 1.0 and q[(3, 3)] == 1.0
    one_user = MR.itemsim(np.array([1, 1]), np.array([1, 2]), np.array([1.0, 1.0]), MR.TANIMOTO)
    assert one_user["sim"].tolist() == [1.0, 1.0]            # 1 / (1 + 1 - 1)
    third = MR.itemsim(np.array([1, 1, 2, 3]), np.array([1, 2, 1, 2]), np.ones(4), MR.TANIMOTO)
    assert third["sim"].tolist() == [1 / 3, 1 / 3]


def test_city_block():
    p = pairs(MR.CITY_BLOCK)
    assert p[(1, 2)] == 1 / (1 + 3 + 3 - 2 * 2)
    assert p[(1, 3)] == 1 / (1 + 3 + 2 - 2 * 1) == p[(3, 2)]


def test_loglikelihood():
    p = pairs(MR.LOGLIKELIHOOD)
    # (1, 2): k = (2, 1, 1, 0): rowE = colE = H(3, 1) = 4 ln 4 - 3 ln 3, matE = H(2, 1, 1, 0) = 4 ln 4 - 2 ln 2
    llr12 = 2 * (10 * math.log(2) - 6 * math.log(3))
    assert p[(1, 2)] == pytest.approx(1 - 1 / (1 + llr12), rel=1e-12)
    assert p[(1, 2)] == pytest.approx(0.40462, abs=5e-6)
    # (1, 3): k = (1, 1, 2, 0): rowE = H(2, 2) = 4 ln 4 - 4 ln 2, colE = H(3, 1), matE = H(1, 1, 2, 0) = 4 ln 4 - 2 ln 2
    llr13 = 2 * ((8 * math.log(2) - 4 * math.log(2)) + (8 * math.log(2) - 3 * math.log(3)) - (8 * math.log(2) - 2 * math.log(2)))
    assert p[(1, 3)] == pytest.approx(1 - 1 / (1 + llr13), rel=1e-12)
    assert p[(1, 3)] == p[(3, 1)]
    # N is the number of users that survive the input preparation: with user 4 dropped the table of (1, 2) is (1, 1, 1, 0)
    keep = U != 4
    r = MR.itemsim(U[keep], I[keep], S[keep], MR.LOGLIKELIHOOD)
    assert r["n_users"] == 3
    llr_small = 2 * (2 * (3 * math.log(3) - 2 * math.log(2)) - 3 * math.log(3))
    got = {(int(a), int(b)): float(s) for a, b, s in zip(r["item"], r["other"], r["sim"])}
    assert got[(1, 2)] == pytest.approx(1 - 1 / (1 + llr_small), rel=1e-12)


def test_euclidean_distance():
    p = pairs(MR.EUCLIDEAN)
    assert p[(1, 2)] == pytest.approx(1 / (1 + math.sqrt(42 - 2 * 18 + 27)), rel=1e-15)      # |(5,4,0,1) - (3,0,3,3)|^2 over all users
    assert p[(1, 3)] == pytest.approx(1 / (1 + math.sqrt(42 - 2 * 16 + 20)), rel=1e-15)
    assert pairs(MR.EUCLIDEAN, exclude_self=False)[(2, 2)] == 1.0


def test_pearson_and_the_constant_item():
    p = pairs(MR.PEARSON)
    # item 2 is rated 3 by everybody: ||c|| = 0, every similarity with it is NaN and dropped
    assert all(2 not in k for k in p)
    # item 1: centre 10 / 3, c = (5, 2, -7) / 3, ||c|| = sqrt(78) / 3; item 3: centre 3, c = (1, -1), ||c|| = sqrt(2); co-rated by u2
    assert p == {(1, 3): pytest.approx(2 / math.sqrt(156), rel=1e-14), (3, 1): pytest.approx(2 / math.sqrt(156), rel=1e-14)}
    assert 2 / math.sqrt(156) == pytest.approx(0.16013, abs=5e-6)
    # a negative correlation fails "sim > 0"
    s2 = S.copy()
    s2[3] = 1.0      # u2 rates item 3 lowest
    r = MR.itemsim(U, I, s2, MR.PEARSON)
    assert len(r["item"]) == 0 and r["corated"] == 6


def test_threshold_top_k_and_ties():
    r = MR.itemsim(U, I, S, MR.TANIMOTO, threshold=0.3)
    assert list(zip(r["item"].tolist(), r["other"].tolist())) == [(1, 2), (2, 1)]
    r = MR.itemsim(U, I, S, MR.TANIMOTO, max_similarities_per_item=1)
    assert list(zip(r["item"].tolist(), r["other"].tolist())) == [(1, 2), (2, 1), (3, 1)]      # (3, 1) and (3, 2) tie: ascending id


@pytest.mark.parametrize("measure,sim_id", [(MR.COSINE, oracle.COSINE), (MR.COOCCURRENCE, oracle.COOCCURRENCE)])
@pytest.mark.parametrize("threshold", [None, 0.15])
def test_statement_equals_the_c_oracle_on_the_golden_matrix(rm_golden, measure, sim_id, threshold):
    user, item, score = rm_golden["coo"]
    keep = score > 0
    user, item, score = user[keep], item[keep], score[keep]
    ref = oracle.itemsim(user, item, score, similarity=sim_id, max_similarities_per_item=10, threshold=threshold)
    got = MR.itemsim(user, item, score, measure, max_similarities_per_item=10, threshold=threshold)
    assert len(got["item"]) == len(ref["item"]) > 0
    assert np.array_equal(got["item"], ref["item"])
    np.testing.assert_allclose(got["sim"], ref["sim"], rtol=1e-12)
    differ = got["other"] != ref["other"]      # only on a near tie may the order differ
    assert np.all(np.abs(got["sim"][differ] - ref["sim"][differ]) <= 1e-12 * np.abs(ref["sim"][differ]))


@pytest.mark.parametrize("measure", MR.MEASURES[2:])
def test_comparator_accepts_the_statement_and_rejects_damage(measure):
    rng = np.random.default_rng(11)
    mask = rng.random((60, 25)) < 0.3
    u, i = np.nonzero(mask)
    u, i = (u + 1).astype(np.int32), (i + 1).astype(np.int32)
    s = rng.integers(1, 6, size=len(u)).astype(np.float32)
    for K, threshold, exclude_self in ((5, None, True), (100, {MR.CITY_BLOCK: 0.05, MR.EUCLIDEAN: 0.05}.get(measure, 0.2), False)):
        ref = MR.itemsim(u, i, s, measure, max_similarities_per_item=K, threshold=threshold, exclude_self=exclude_self)
        rows = {"item": ref["item"], "other": ref["other"], "sim": ref["sim"].astype(np.float32)}
        info = MR.check_rows(rows, u, i, s, measure, K, exclude_self=exclude_self, threshold=threshold)
        assert info["rows"] > 0 and info["corated"] == ref["corated"]
        bad = dict(rows, sim=rows["sim"].copy())
        bad["sim"][0] *= np.float32(1.001)
        with pytest.raises(AssertionError):
            MR.check_rows(bad, u, i, s, measure, K, exclude_self=exclude_self, threshold=threshold)
        short = {k: v[1:] for k, v in rows.items()}      # the best entry of the first row is missing
        with pytest.raises(AssertionError):
            MR.check_rows(short, u, i, s, measure, K, exclude_self=exclude_self, threshold=threshold)


def test_names_of_the_python_host():
    host = __import__("importlib").import_module("filmyou-core_amd.host")
    P = pkg()
    names = [P.SIMILARITY_COSINE, P.SIMILARITY_COOCCURRENCE, P.SIMILARITY_TANIMOTO_COEFFICIENT, P.SIMILARITY_LOGLIKELIHOOD,
             P.SIMILARITY_CITY_BLOCK, P.SIMILARITY_EUCLIDEAN_DISTANCE, P.SIMILARITY_PEARSON_CORRELATION]
    assert names == list(MR.MEASURES)
    assert [host.similarity_id(n) for n in names] == list(range(7))
    package = "org.apache.mahout.math.hadoop.similarity.cooccurrence.measures."
    classes = ["CosineSimilarity", "CooccurrenceCountSimilarity", "TanimotoCoefficientSimilarity", "LoglikelihoodSimilarity",
               "CityBlockSimilarity", "EuclideanDistanceSimilarity", "PearsonCorrelationSimilarity"]
    assert [host.similarity_id(package + c) for c in classes] == list(range(7))
    assert [host.similarity_id("class " + package + c) for c in classes] == list(range(7))      # String.valueOf(X.class)
    for bad in ("class org.apache.mahout...CooccurrenceCountSimilarity", "SIMILARITY_JACCARD", package, "class ", package + "Cosine", None, 3):
        with pytest.raises(ValueError):
            host.similarity_id(bad)


def test_header_declares_the_enum_in_mahouts_order():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "filmyou.h")).read()
    found = dict(re.findall(r"FY_(SIMILARITY_[A-Z_]+) = (\d)", text))
    assert found == {name: str(k) for k, name in enumerate(MR.MEASURES)}


def test_names_of_the_cpp_mirror(tmp_path):
    """fy::host::RowSimilarityJob::similarityId (filmyou-core_amd/host/filmyou_job.hpp) is a third hand-written copy of the table:
    a small host program prints what it maps every spelling to (header-only use: nothing of the library is called)."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the C++ mirror")
    package = "org.apache.mahout.math.hadoop.similarity.cooccurrence.measures."
    classes = ["CosineSimilarity", "CooccurrenceCountSimilarity", "TanimotoCoefficientSimilarity", "LoglikelihoodSimilarity",
               "CityBlockSimilarity", "EuclideanDistanceSimilarity", "PearsonCorrelationSimilarity"]
    good = list(MR.MEASURES) + [package + c for c in classes] + ["class " + package + c for c in classes]
    bad = ["class org.apache.mahout...CooccurrenceCountSimilarity", "SIMILARITY_JACCARD", package, "class ", package + "Cosine", ""]
    src = tmp_path / "names.cpp"
    src.write_text("""#include <cstdio>
#include <stdexcept>
#include "filmyou_job.hpp"
int main(int argc, char** argv) {
    for (int k = 1; k < argc; k++) {
        try { std::printf("%d\\n", fy::host::RowSimilarityJob::similarityId(argv[k])); }
        catch (const std::invalid_argument&) { std::printf("invalid\\n"); }
    }
    return 0;
}
""")
    exe = tmp_path / "names"
    lib_dir = os.path.dirname(pkg().LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "filmyou-core_amd", "host"), "-I", os.path.join(root, "include"),
                    "-o", str(exe), str(src), "-L" + lib_dir, "-lfilmyou_hip", "-Wl,-rpath," + lib_dir], check=True)
    out = subprocess.run([str(exe)] + good + bad, check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(k) for k in range(7)] * 3 + ["invalid"] * len(bad)
