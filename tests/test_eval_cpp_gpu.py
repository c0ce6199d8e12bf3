"""Offline evaluation through the C++ host-side mirror (fy::host::Evaluator, fy::host::holdout, RM2Job::runEvaluated): the compiled
driver links only the C ABI; on the reference's fixture, split at fraction 0.2 / seed 1, its `eval` line is the Python evaluation of the
same job -- with the test ratings from a file and with the split made by the driver itself."""
import re
import subprocess

import numpy as np
import pytest

from test_eval_gpu import fixture, fixture_conf, split_fixture
from util import pkg

pytestmark = pytest.mark.gpu

EVAL_LINE = re.compile(r"eval lists (\d+) users_evaluated (\d+) lists_without_relevant (\d+) relevant_users (\d+) relevant_entries (\d+) cutoff (\d+) "
                       r"hits (\d+) users_hit (\d+) precision (\S+) recall (\S+) map (\S+) mrr (\S+) ndcg (\S+)")


@pytest.mark.parametrize("cutoff", [1, 10])
def test_cpp_evaluate_equals_the_python_evaluation(tmp_path, cutoff):
    P = pkg()
    exe = P._native.build_host_driver()
    g = fixture()
    ctx = P.Context(0)
    train, test, _ = split_fixture(P, ctx, g)
    E = P.Evaluator(ctx, test, cutoffs=(cutoff,), relevance_threshold=4.0)
    rec = P.RM2Job(fixture_conf(P, g), ctx).run(train, clustering=g["map"])
    ev = E.evaluate(rec)
    means = ev.means()
    want_int = [ev.lists, ev.users_evaluated, ev.lists_without_relevant, ev.relevant_users, ev.relevant_entries, cutoff, int(ev.hits[0]), int(ev.users_hit[0])]
    want_mean = [float(means[k][0]) for k in ("precision", "recall", "map", "mrr", "ndcg")]
    assert ev.hits[0] > 0
    fmt = ["%d", "%d", "%.1f"]
    np.savetxt(tmp_path / "all.txt", np.c_[g["kept"]], fmt=fmt)
    np.savetxt(tmp_path / "train.txt", np.c_[train.to_host()], fmt=fmt)
    np.savetxt(tmp_path / "test.txt", np.c_[test.to_host()], fmt=fmt)
    np.savetxt(tmp_path / "clustering.txt", np.c_[g["map"]], fmt="%d")
    for x in (rec, E, train, test):
        x.close()
    ctx.close()
    job = [str(tmp_path / "clustering.txt"), "0.5", str(g["numberOfItems"]), str(g["numberOfClusters"]), "1000"]
    for args in (["--evaluate", str(tmp_path / "test.txt"), str(cutoff), str(tmp_path / "train.txt")],
                 ["--evaluate", "holdout:0.2:1", str(cutoff), str(tmp_path / "all.txt")]):
        out = subprocess.run([exe] + args + job, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        m = EVAL_LINE.search(out.stderr)
        assert m, out.stderr
        assert list(map(int, m.groups()[:8])) == want_int
        got = np.array(list(map(float, m.groups()[8:])))
        assert np.all(np.abs(got - want_mean) <= 1e-12 * np.abs(want_mean)), (got, want_mean)
        assert len(out.stdout.strip().splitlines()) == rec.size
        if args[1].startswith("holdout"):
            assert "holdout train %d test 507" % (2489 - 507) in out.stderr
