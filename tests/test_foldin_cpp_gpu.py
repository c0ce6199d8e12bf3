"""The C++ host mirror of the fold-in (fy::host::FoldIn through `rm2_main --fold-in`) on the reference's PPC data: the factor rows and
clusters of the numpy statement (tests/foldin_ref.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import foldin_ref as FR
from util import pkg

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factorization_test_data.json")


def test_cpp_fold_in_prints_the_statements_rows(tmp_path):
    P = pkg()
    exe = P._native.build_host_driver()
    with open(GOLDEN) as f:
        d = json.load(f)["ppc"]
    W = np.array(d["W_ten"])                                  # the standing factors of the ten-iteration run
    profiles = [(l, it, sc, np.zeros(len(it), np.uint8)) for l, it, sc in FR.profiles_of_columns(d["A"])]
    profiles.append((77, [3, 3, 0, 5, 8, 8], [1.0, 2.0, 4.0, 0.0, 3.0, 0.0], [0, 0, 0, 0, 0, 1]))      # duplicate, outside id, score <= 0, delete
    profiles.append((78, [101, 4], [3.0, 1.0], [0, 1]))                                                  # composes to nothing
    with open(tmp_path / "profiles.txt", "w") as f:
        for label, items, scores, remove in profiles:
            for it, sc, rm in zip(items, scores, remove):
                f.write("%d %d %s\n" % (label, it, "x" if rm else "%.9g" % sc))      # "x" is the delete marker
    np.savetxt(tmp_path / "W.txt", W, fmt="%.17g")
    ref = FR.assign(W, profiles, iterations=10, ppc=True, f=12)
    out = subprocess.run([exe, "--fold-in", str(tmp_path / "profiles.txt"), str(tmp_path / "W.txt"), "10", "10", "1", "12"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = [l.split() for l in out.stdout.strip().splitlines()]
    rows = [r for r in rows if len(r) == 13]
    assert [int(r[0]) for r in rows] == ref["labels"].tolist()
    compared = ref["status"] == FR.OK
    assert all(m > 1e-9 for m, c in zip(ref["margin"], compared) if c)
    np.testing.assert_allclose(np.array([[float(x) for x in r[3:]] for r in rows]), ref["H"], rtol=1e-10, atol=1e-300)
    assert [int(r[1]) for r in rows] == ref["clusters"].tolist() and [int(r[2]) for r in rows] == ref["status"].tolist()
    assert ref["status"][30:].tolist() == [FR.OK, FR.EMPTY]
    assert "foldin asked 32 assigned 31 empty 1" in out.stderr and "out_of_range 2 superseded 2 removed 2 nonpositive 1" in out.stderr
