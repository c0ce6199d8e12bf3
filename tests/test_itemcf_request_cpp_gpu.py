"""The C++ host mirror's BaselineRecommenderJob::prepare / recommendUsers through the host driver's --recommend-users mode (a
compiled program that links only the C ABI): its printed rows, parsed back to float32, are bitwise the Python request's."""
import subprocess

import numpy as np
import pytest

import itemsim_measures_ref as MR
from test_itemcf_filter_gpu import bits, user_request
from util import pkg, synth

pytestmark = pytest.mark.gpu


def test_cpp_recommend_users_prints_the_python_requests_rows(tmp_path):
    P = pkg()
    exe = P._native.build_host_driver()
    u, i, s, _ = synth().generate("tiny")
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    users = user_request(u, np.random.default_rng(41), share=0.15)
    np.savetxt(tmp_path / "ratings.txt", np.c_[u, i, s], fmt=["%d", "%d", "%.1f"])
    (tmp_path / "users.txt").write_text("\n".join(str(int(x)) for x in users) + "\n")
    out = subprocess.run([exe, "--recommend-users", str(tmp_path / "users.txt"), str(tmp_path / "ratings.txt"), "SIMILARITY_LOGLIKELIHOOD", "15",
                          "10", "10"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    with P.Context(0) as ctx:
        prepared = P.BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=15, similarityClassname=MR.LOGLIKELIHOOD)
        want = prepared.recommend(users, numRecommendations=10, maxPrefsPerUser=10)
        rows, rq = want.rows(), want.request_stats
        prepared.close()
    assert "request users_known %d items_needed %d rows_built %d " % (rq["users_known"], rq["items_needed"], rq["rows_built"]) in out.stderr
    lines = [l.split() for l in out.stdout.strip().splitlines()]
    got = {"user": np.array([int(a) for a, _, _ in lines], dtype=np.int32), "item": np.array([int(b) for _, b, _ in lines], dtype=np.int32),
           "score": np.array([float(c) for _, _, c in lines], dtype=np.float32)}
    assert len(rows["user"]) > 0 and bits(got) == bits(rows)
