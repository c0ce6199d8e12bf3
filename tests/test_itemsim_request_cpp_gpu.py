"""The C++ host mirror's RowSimilarityJob::runItems through the host driver's --similar-items mode (a compiled program that links
only the C ABI): its printed rows, parsed back to float32, are bitwise the Python request's."""
import subprocess

import numpy as np
import pytest

import itemsim_measures_ref as MR
from util import pkg, synth

pytestmark = pytest.mark.gpu


def test_cpp_similar_items_prints_the_python_requests_rows(tmp_path):
    P = pkg()
    exe = P._native.build_host_driver()
    u, i, s, _ = synth().generate("tiny")
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    rng = np.random.default_rng(41)
    ids = np.concatenate([rng.choice(np.unique(i), size=40, replace=False), [0, -5, 100000]]).astype(np.int32)
    np.savetxt(tmp_path / "ratings.txt", np.c_[u, i, s], fmt=["%d", "%d", "%.1f"])
    (tmp_path / "items.txt").write_text("\n".join(str(int(x)) for x in ids) + "\n")
    out = subprocess.run([exe, "--similar-items", str(tmp_path / "items.txt"), str(tmp_path / "ratings.txt"), "SIMILARITY_LOGLIKELIHOOD", "20"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "request items_known 40 " in out.stderr
    lines = [l.split() for l in out.stdout.strip().splitlines()]
    got = {"item": np.array([int(a) for a, _, _ in lines], dtype=np.int32), "other": np.array([int(b) for _, b, _ in lines], dtype=np.int32),
           "sim": np.array([float(c) for _, _, c in lines], dtype=np.float32)}
    with P.Context(0) as ctx:
        job = P.RowSimilarityJob(ctx).prepare((u, i, s), similarityClassname=MR.LOGLIKELIHOOD, maxSimilaritiesPerRow=20)
        want = job.rows(ids).rows()
        job.close()
    assert len(want["item"]) > 0
    assert np.array_equal(got["item"], want["item"]) and np.array_equal(got["other"], want["other"])
    assert np.array_equal(got["sim"].view(np.uint32), want["sim"].view(np.uint32))
