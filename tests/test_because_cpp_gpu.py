"""Explanations through the C++ host-side mirror (BaselineRecommenderJob::recommendedBecause) and the host driver's --because mode (a
compiled program that links only the C ABI): on the reference's fixture its printed rows, parsed back to float32, are bitwise the
rows of the Python call, and its `because` line carries the Python counters."""
import re
import subprocess

import numpy as np
import pytest

import itemsim_measures_ref as MR
from test_itemcf_filter_gpu import golden_data
from util import pkg

pytestmark = pytest.mark.gpu

LINE = re.compile(r"because pairs (\d+) rows (\d+) contributors (\d+) ok (\d+) unknown_user (\d+) unknown_item (\d+) own_preference (\d+) too_few (\d+) "
                  r"zero_numerator (\d+) not_a_number (\d+) users_known (\d+) targets (\d+) rows_built (\d+) row_entries_walked (\d+)")


def test_cpp_because_prints_the_python_rows(tmp_path, rm_golden):
    P = pkg()
    exe = P._native.build_host_driver()
    u, i, s = golden_data(rm_golden)
    users = np.concatenate([np.unique(u)[::3], [7, -2]]).astype(np.int32)          # an unknown user and a negative id among them
    items = np.concatenate([np.unique(i)[::4], [13]]).astype(np.int32)             # an item nobody rated
    pu, pi = (a.ravel().astype(np.int32) for a in np.meshgrid(users, items, indexing="ij"))
    with P.Context(0) as ctx:
        prepared = P.BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=20, similarityClassname=MR.LOGLIKELIHOOD)
        bec = prepared.because((pu, pi), howMany=3, maxPrefsPerUser=8)
        rows, pairs, st = bec.rows(), bec.pairs(), bec.because_stats
        bec.close()
        prepared.close()
    assert len(rows["pair"]) > 100 and (pairs["status"] == 0).any() and (pairs["status"] == 1).any() and (pairs["status"] == 2).any()
    np.savetxt(tmp_path / "ratings.txt", np.c_[u, i, s], fmt=["%d", "%d", "%.1f"])
    np.savetxt(tmp_path / "pairs.txt", np.c_[pu, pi], fmt="%d")
    out = subprocess.run([exe, "--because", str(tmp_path / "pairs.txt"), str(tmp_path / "ratings.txt"), "SIMILARITY_LOGLIKELIHOOD", "20", "8", "3"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    m = LINE.search(out.stderr)
    assert m, out.stderr
    assert list(map(int, m.groups())) == [st["pairs_asked"], st["rows"], st["contributors"]] + st["by_status"][:7] + [
        st["users_known"], st["targets"], st["rows_built"], st["row_entries_walked"]]
    lines = [l.split() for l in out.stdout.strip().splitlines()]
    listed = [l for l in lines if l[0] != "#"]
    per_pair = [l[1:] for l in lines if l[0] == "#"]
    for col, name in enumerate(("pair", "user", "item", "because")):
        assert [int(l[col]) for l in listed] == rows[name].tolist(), name
    for col, name in ((4, "sim"), (5, "pref")):
        printed = np.array([float(l[col]) for l in listed], dtype=np.float32)
        assert np.array_equal(printed.view(np.uint32), rows[name].view(np.uint32)), name
    assert [int(l[0]) for l in per_pair] == list(range(len(pu)))
    for col, name in ((1, "user"), (2, "item"), (4, "status"), (5, "contributors")):
        assert [int(l[col]) for l in per_pair] == pairs[name].tolist(), name
    printed = np.array([float(l[3]) for l in per_pair], dtype=np.float32)
    ok = pairs["status"] == 0
    assert np.array_equal(printed.view(np.uint32)[ok], pairs["estimate"].view(np.uint32)[ok]) and np.isnan(printed[~ok]).all()
    # the driver refuses what the call refuses
    bad = subprocess.run([exe, "--because", str(tmp_path / "pairs.txt"), str(tmp_path / "ratings.txt"), "SIMILARITY_LOGLIKELIHOOD", "20", "8", "65"],
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1 and "howMany" in bad.stderr
