"""Ratings that take writes through the C++ host-side mirror (fy::host::applyWrites): the compiled driver links only the C ABI; on
the reference's fixture, damaged and restored by a batch, its rows are the golden triples."""
import re
import subprocess

import numpy as np
import pytest

from test_ratings_update_gpu import damaged_fixture
from util import RTOL, pkg

pytestmark = pytest.mark.gpu


def test_cpp_apply_writes_against_the_golden_triples(tmp_path, rm_golden):
    P = pkg()
    exe = P._native.build_host_driver()
    g = rm_golden
    (u, i, s), (bu, bi, bs, br), want = damaged_fixture(g)
    np.savetxt(tmp_path / "ratings.txt", np.c_[u, i, s], fmt=["%d", "%d", "%.1f"])
    np.savetxt(tmp_path / "writes.txt", np.c_[bu, bi, bs, br], fmt=["%d", "%d", "%.1f", "%d"])
    np.savetxt(tmp_path / "clustering.txt", np.c_[g["map_user"], g["map_cluster"]], fmt="%d")
    out = subprocess.run([exe, "--writes", str(tmp_path / "writes.txt"), str(tmp_path / "ratings.txt"), str(tmp_path / "clustering.txt"),
                          "0.5", "100", "10", "1000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    m = re.search(r"writes (\d+) superseded (\d+) replaced (\d+) inserted (\d+) deleted (\d+) delete_missed (\d+) source_dropped (\d+) nnz_out (\d+)",
                  out.stderr)
    assert m, out.stderr
    assert list(map(int, m.groups())) == [want[k] for k in ("n_writes", "n_superseded", "n_replaced", "n_inserted", "n_deleted", "n_delete_missed",
                                                            "n_source_dropped", "nnz_out")]
    rows = [l.split() for l in out.stdout.strip().splitlines()]
    got = {(int(a), int(b)): float(c) for a, b, c, _ in rows}
    exp = np.asarray(g["recommendations"])
    assert len(rows) == len(got) == len(exp) == 507
    for a, b, c in exp:
        assert abs(got[(int(a), int(b))] - c) <= RTOL * abs(c)
