"""The C++ host mirror's BaselineRecommenderJob::recommendProfiles through the host driver's --recommend-profiles mode (a compiled
program that links only the C ABI): its printed rows, parsed back to float32, are bitwise the Python call's, for both bases."""
import subprocess

import numpy as np
import pytest

import itemsim_measures_ref as MR
from test_itemcf_filter_gpu import bits
from util import pkg, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("base", ["whole", "resident"])
def test_cpp_recommend_profiles_prints_the_python_calls_rows(tmp_path, base):
    P = pkg()
    exe = P._native.build_host_driver()
    u, i, s, _ = synth().generate("tiny")
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    rng = np.random.default_rng(8)
    known = np.unique(u)
    profiles = []
    for x in rng.choice(known, size=12, replace=False).tolist() + [int(known.max()) + 9]:
        m = u == x
        it, sc = i[m], s[m]
        if base == "whole":          # the user's own ratings in shuffled order, one of them written twice, an unknown item
            order = rng.permutation(len(it))
            items = [int(i.max()) + 5] + it[order].tolist() + it[order][:1].tolist()
            scores = [2.0] + sc[order].tolist() + [0.5] * min(1, len(it))
            remove = [0] * len(items)
        else:                        # writes on the resident row: an upsert, a delete of an item of the row, a delete of an absent item
            others = np.setdiff1d(np.unique(i), it)
            items = ([int(it[0]), int(it[-1])] if len(it) else []) + [int(others[0]), int(others[1])]
            scores = ([1.5, 0.0] if len(it) else []) + [4.5, 0.0]
            remove = ([0, 1] if len(it) else []) + [0, 1]
        profiles.append((x, items, scores, remove))
    np.savetxt(tmp_path / "ratings.txt", np.c_[u, i, s], fmt=["%d", "%d", "%.1f"])
    lines = ["%d %d %s" % (x, it, "x" if gone else "%.1f" % sc) for x, items, scores, remove in profiles for it, sc, gone in zip(items, scores, remove)]
    (tmp_path / "profiles.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, "--recommend-profiles", str(tmp_path / "profiles.txt"), "--profile-base", base, str(tmp_path / "ratings.txt"),
                          "SIMILARITY_LOGLIKELIHOOD", "15", "10", "10"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    with P.Context(0) as ctx:
        prepared = P.BaselineRecommenderJob(ctx).prepare((u, i, s), maxSimilaritiesPerItem=15, similarityClassname=MR.LOGLIKELIHOOD)
        want = prepared.recommend_profiles(profiles, numRecommendations=10, maxPrefsPerUser=10, base=base)
        rows, ps = want.rows(), want.profile_stats
        prepared.close()
    assert ("profiles asked %d scored %d empty %d users_unknown %d entries %d unknown_item %d superseded %d removes_hit %d removes_missed %d prefs_composed %d "
            "items_needed %d rows_built %d" % (ps["profiles_asked"], ps["profiles_scored"], ps["profiles_empty"], ps["users_unknown"], ps["entries"],
                                                ps["entries_unknown_item"], ps["entries_superseded"], ps["removes_hit"], ps["removes_missed"],
                                                ps["prefs_composed"], ps["items_needed"], ps["rows_built"])) in out.stderr
    assert ps["entries"] == len(lines) and (ps["users_unknown"] == 1) == (base == "resident")
    parsed = [l.split() for l in out.stdout.strip().splitlines()]
    got = {"user": np.array([int(a) for a, _, _ in parsed], dtype=np.int32), "item": np.array([int(b) for _, b, _ in parsed], dtype=np.int32),
           "score": np.array([float(c) for _, _, c in parsed], dtype=np.float32)}
    assert len(rows["user"]) > 0 and bits(got) == bits(rows)
