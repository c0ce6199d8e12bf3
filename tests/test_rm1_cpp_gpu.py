"""The RM1 estimator through the C++ host-side mirror: the compiled driver (which links only the C ABI) with a trailing
relevanceModel=rm1 gives the Python host's rows bit for bit, for the whole job and for a usersFile; a bad value is refused."""
import os
import subprocess

import numpy as np
import pytest

from rm1_definition import definition_full
from util import assert_topn_matches, pkg, synth

pytestmark = pytest.mark.gpu


def parse(stdout):
    got = np.array([l.split() for l in stdout.strip().splitlines()])
    return {"user": got[:, 0].astype(np.int32), "item": got[:, 1].astype(np.int32),
            "score": got[:, 2].astype(np.float64).astype(np.float32),      # %.9g reads back exactly
            "cluster": got[:, 3].astype(np.int32)}


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int32) if k == "score" else a[k], b[k].view(np.int32) if k == "score" else b[k])
               for k in ("user", "item", "score", "cluster"))


def test_cpp_driver_with_the_rm1_key_gives_the_python_rows(tmp_path):
    P = pkg()
    S = synth()
    exe = P._native.build_host_driver()
    u, i, s, facts = S.generate("tiny")
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    uu = np.unique(u)
    clustering = (uu, S.hash_clustering(uu, 7))
    np.savetxt(tmp_path / "ratings.txt", np.c_[u, i, s], fmt=["%d", "%d", "%.1f"])
    np.savetxt(tmp_path / "clustering.txt", np.c_[clustering[0], clustering[1]], fmt="%d")
    conf = P.Configuration()
    for k, v in (("relevanceModel", "rm1"), ("smoothing", "dirichlet"), ("mu", "100"), ("numberOfItems", str(facts["n_items"])), ("numberOfClusters", "7"),
                 ("numberOfRecommendations", "10")):
        conf.set(k, v)
    ctx = P.Context(0)
    rows = P.RM2Job(conf, ctx).run((u, i, s), clustering=clustering).rows()
    assert_topn_matches(rows, definition_full(u, i, s, "dirichlet", 100.0, clustering=clustering), 10)
    base = [str(tmp_path / "ratings.txt"), str(tmp_path / "clustering.txt"), "0.1", str(facts["n_items"]), "7", "10"]
    keys = ["smoothing=dirichlet", "mu=100", "relevanceModel=RM1"]
    out = subprocess.run([exe] + base + keys, capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert out.returncode == 0, out.stderr
    assert len(rows["user"]) > 0 and same_bits(parse(out.stdout), rows)
    # the usersFile of the mirror follows the job's estimator
    asked = [int(uu[5]), int(uu[40]), int(uu[5]), 10 ** 6]
    (tmp_path / "users.txt").write_text("".join("%d\n" % x for x in asked))
    out = subprocess.run([exe, "--users", str(tmp_path / "users.txt")] + base + keys, capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert out.returncode == 0, out.stderr
    keep = np.isin(rows["user"], asked)
    assert keep.sum() == 20 and same_bits(parse(out.stdout), {k: rows[k][keep] for k in rows})
    # without the key the driver runs RM2: other scores
    out = subprocess.run([exe] + base + keys[:2], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert out.returncode == 0 and not np.array_equal(parse(out.stdout)["score"], rows["score"])
    bad = subprocess.run([exe] + base + ["relevanceModel=rm3"], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert bad.returncode == 1 and "relevanceModel" in bad.stderr, bad.stderr
    ctx.close()
