"""RM2 lists for given profiles through the C++ host-side mirror (fy::host::RM2Job::scoreProfiles, rm2_main --score-profiles) on
the reference's fixture: the compiled driver links only the C ABI; its rows are the plain statement's (tests/rm2_profile_ref.py)."""
import re
import subprocess

import numpy as np
import pytest

import rm2_profile_ref as RP
from util import RTOL, assert_topn_matches, pkg

pytestmark = pytest.mark.gpu

TOP_N = 10


def run_driver(tmp_path, g, profiles, base, cluster=None):
    exe = pkg()._native.build_host_driver()
    u, i, s = g["coo"]
    np.savetxt(tmp_path / "ratings.txt", np.c_[u, i, s], fmt=["%d", "%d", "%.1f"])
    np.savetxt(tmp_path / "clustering.txt", np.c_[g["map_user"], g["map_cluster"]], fmt="%d")
    lines = []
    for label, items, scores, remove in profiles:
        lines += ["%d %d %s" % (label, it, "x" if rm else repr(float(sc))) for it, sc, rm in zip(items, scores, remove)]
    (tmp_path / "profiles.txt").write_text("\n".join(lines) + "\n")
    args = [exe, "--score-profiles", str(tmp_path / "profiles.txt"), "--profile-base", base]
    if cluster is not None:
        args += ["--profile-cluster", str(cluster)]
    out = subprocess.run(args + [str(tmp_path / "ratings.txt"), str(tmp_path / "clustering.txt"), "0.5", "100", "10", str(TOP_N)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = [l.split() for l in out.stdout.strip().splitlines()]
    m = re.search(r"profiles asked (\d+) scored (\d+) empty (\d+) users_unknown (\d+) users_filtered (\d+) entries (\d+) unknown_item (\d+) "
                  r"nonpositive (\d+) superseded (\d+) removes_hit (\d+) removes_missed (\d+) items_composed (\d+) clusters_touched (\d+) "
                  r"slab_rows (\d+)", out.stderr)
    assert m, out.stderr
    keys = ("profiles_asked", "profiles_scored", "profiles_empty", "users_unknown", "users_filtered", "entries", "entries_unknown_item",
            "entries_nonpositive", "entries_superseded", "removes_hit", "removes_missed", "items_composed", "clusters_touched", "slab_rows")
    return ({"label": np.array([int(r[0]) for r in rows]), "item": np.array([int(r[1]) for r in rows], dtype=np.int32),
             "score": np.array([float(r[2]) for r in rows], dtype=np.float32), "cluster": np.array([int(r[3]) for r in rows], dtype=np.int32)},
            dict(zip(keys, map(int, m.groups()))))


def compare(rows, counters, model, profiles, base, clusters=None):
    composed, c = RP.compose(model, profiles, base, clusters=clusters)
    groups, ref = RP.score(model, composed, base)
    counts = [min(TOP_N, len(g[2])) for g in groups]
    assert len(rows["label"]) == sum(counts) > 0 and counters["profiles_scored"] == len(groups)
    assert np.array_equal(rows["label"], np.concatenate([np.full(n, g[0]) for n, g in zip(counts, groups)]))
    for k in RP.COUNTERS:
        if k not in ("profiles_scored", "profiles_mine"):
            assert counters[k] == c[k], (k, counters[k], c[k])
    got = dict(rows)
    got["user"] = np.concatenate([np.full(n, k) for k, n in enumerate(counts)]).astype(np.int32)
    assert_topn_matches(got, ref, TOP_N, rtol=RTOL)


def test_cpp_score_profiles_prints_the_statements_rows(tmp_path, rm_golden):
    g = rm_golden
    u, i, s = g["coo"]
    model = RP.Model(u, i, s, 0.5, g["numberOfItems"], (g["map_user"], g["map_cluster"]))
    # resident: pending writes of three users (one twice in a row would merge, so the repeat comes later), an unknown user
    profiles = []
    for x in (17, 3, 29, 1000, 17):
        if x not in model.cluster_of:
            profiles.append((x, [1], [2.0], [0]))
            continue
        K = model.clusters[model.cluster_of[x]]
        own = K["items"][K["rated"][K["row"][x]]].tolist()
        absent = sorted(set(K["items"].tolist()) - set(own))
        k = len(profiles)
        profiles.append((x, [absent[k], own[k], absent[k], 5000, own[k + 1]], [3.0, 0.0, 1.0, 2.0, 0.0], [0, 1, 0, 0, 0]))
    rows, counters = run_driver(tmp_path, g, profiles, "resident")
    compare(rows, counters, model, profiles, "resident")
    assert counters["users_unknown"] == 1 and counters["removes_hit"] == 4 and counters["entries_nonpositive"] == 4
    # whole: three visitors scored in cluster 3
    items = model.clusters[3]["items"].tolist()
    whole = [(-1, items[:4], [1.0] * 4, [0] * 4), (-2, items[5:6], [2.5], [0]), (-1, items[2:9] + items[2:3], [1.0] * 7 + [0.0], [0] * 7 + [1])]
    rows, counters = run_driver(tmp_path, g, whole, "whole", cluster=3)
    compare(rows, counters, model, whole, "whole", clusters=[3, 3, 3])
    assert set(rows["cluster"].tolist()) == {3} and counters["clusters_touched"] == 1 and counters["removes_missed"] == 1
