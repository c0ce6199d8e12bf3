"""Estimated preferences through the C++ host-side mirror (BaselineRecommenderJob::estimatePairs, fy::host::estimateErrors) and the
host driver's --estimate-pairs mode (a compiled program that links only the C ABI): on the reference's fixture, split at fraction
0.2 / seed 1, its printed rows, parsed back to float32, are bitwise the Python estimates, and its `estimate` line carries the Python
error counters and means -- with the test ratings from a file and with the split made by the driver itself."""
import re
import subprocess

import numpy as np
import pytest

import itemsim_measures_ref as MR
from test_itemcf_filter_gpu import golden_data
from util import pkg

pytestmark = pytest.mark.gpu

LINE = re.compile(r"estimate pairs (\d+) estimated (\d+) truth_not_finite (\d+) ok (\d+) unknown_user (\d+) unknown_item (\d+) own_preference (\d+) "
                  r"too_few (\d+) zero_numerator (\d+) not_a_number (\d+) row_entries_walked (\d+) mae (\S+) rmse (\S+)")


def test_cpp_estimate_pairs_prints_the_python_estimates(tmp_path, rm_golden):
    P = pkg()
    exe = P._native.build_host_driver()
    u, i, s = golden_data(rm_golden)
    with P.Context(0) as ctx:
        R = P.Ratings(ctx, u, i, s)
        train, test = R.holdout(0.2, seed=1)
        prepared = P.BaselineRecommenderJob(ctx).prepare(train, maxSimilaritiesPerItem=20, similarityClassname=MR.LOGLIKELIHOOD)
        est = prepared.estimate(test, maxPrefsPerUser=8)
        rows, err, walked = est.rows(), est.errors(test), est.estimate_stats["row_entries_walked"]
        fmt = ["%d", "%d", "%.1f"]
        np.savetxt(tmp_path / "all.txt", np.c_[u, i, s], fmt=fmt)
        np.savetxt(tmp_path / "train.txt", np.c_[train.to_host()], fmt=fmt)
        np.savetxt(tmp_path / "test.txt", np.c_[test.to_host()], fmt=fmt)
        n_train = train.nnz
        for x in (est, prepared, train, test, R):
            x.close()
    assert err.estimated >= 50 and err.pairs == len(rows["user"]) > err.estimated
    want_int = [err.pairs, err.estimated, err.truth_not_finite] + err.by_status[:7] + [walked]
    for args in ([str(tmp_path / "test.txt"), str(tmp_path / "train.txt")], ["holdout:0.2:1", str(tmp_path / "all.txt")]):
        out = subprocess.run([exe, "--estimate-pairs"] + args + ["SIMILARITY_LOGLIKELIHOOD", "20", "8"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        m = LINE.search(out.stderr)
        assert m, out.stderr
        assert list(map(int, m.groups()[:11])) == want_int
        got = np.array(list(map(float, m.groups()[11:])))
        assert np.array_equal(got, np.array([err.mae, err.rmse])), (got, err.mae, err.rmse)          # %.17g: the same doubles
        lines = [l.split() for l in out.stdout.strip().splitlines()]
        assert [int(l[0]) for l in lines] == rows["user"].tolist() and [int(l[1]) for l in lines] == rows["item"].tolist()
        assert [int(l[3]) for l in lines] == rows["status"].tolist()
        printed = np.array([float(l[2]) for l in lines], dtype=np.float32)
        assert np.array_equal(printed.view(np.uint32)[rows["status"] == 0], rows["estimate"].view(np.uint32)[rows["status"] == 0])
        assert np.isnan(printed[rows["status"] != 0]).all()
        if args[0].startswith("holdout"):
            assert "holdout train %d test %d" % (n_train, err.pairs) in out.stderr
