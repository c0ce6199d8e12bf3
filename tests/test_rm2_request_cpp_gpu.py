"""RM2 on request through the C++ host-side mirror (fy::host::RM2Job::runUsers, the usersFile key) on the reference's fixture:
the compiled driver links only the C ABI; its rows are the golden triples of the listed users."""
import os
import re
import subprocess

import numpy as np
import pytest

from util import RTOL, pkg

pytestmark = pytest.mark.gpu


def test_cpp_users_file_against_the_golden_triples(tmp_path, rm_golden):
    P = pkg()
    exe = P._native.build_host_driver()
    g = rm_golden
    u, i, s = g["coo"]
    np.savetxt(tmp_path / "ratings.txt", np.c_[u, i, s], fmt=["%d", "%d", "%.1f"])
    np.savetxt(tmp_path / "clustering.txt", np.c_[g["map_user"], g["map_cluster"]], fmt="%d")
    asked = [17, 3, 3, 29, 0, -4, 1000]
    (tmp_path / "users.txt").write_text("".join("%d\n" % x for x in asked) + "\nabc\n")
    out = subprocess.run([exe, "--users", str(tmp_path / "users.txt"), str(tmp_path / "ratings.txt"), str(tmp_path / "clustering.txt"),
                          "0.5", "100", "10", "1000"], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, FY_REQ_FULL_SHARE="2"))      # the restricted pass, not the full-pass fallback
    assert out.returncode == 0, out.stderr
    rows = [l.split() for l in out.stdout.strip().splitlines()]
    got = {(int(a), int(b)): float(c) for a, b, c, _ in rows}
    exp = [(int(a), int(b), c) for a, b, c in np.asarray(g["recommendations"]) if int(a) in (3, 17, 29)]
    assert len(rows) == len(got) == len(exp) > 0
    for a, b, c in exp:
        assert abs(got[(a, b)] - c) <= RTOL * abs(c)
    m = re.search(r"request users_known (\d+) clusters_touched (\d+) slab_rows (\d+) full_pass_clusters (\d+)", out.stderr)
    assert m, out.stderr
    known, touched, slab_rows, full_pass = map(int, m.groups())
    assert known == 3 and touched >= 1 and slab_rows > 0 and full_pass == 0
