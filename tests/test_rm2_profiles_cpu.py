"""RM2 lists for given profiles, the parts that need no GPU: the plain statement (tests/rm2_profile_ref.py) pinned to the
reference's golden rows, every composition rule and counter of it on hand cases, the ABI additions and the host layer's packing."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import rm2_profile_ref as RP
from util import RTOL, pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fy_rm2_score_profiles", "fy_result_rm2_profile_stats")


def golden_model(g):
    u, i, s = g["coo"]
    return RP.Model(u, i, s, g["params"]["lambda"], g["numberOfItems"], (g["map_user"], g["map_cluster"]))


def test_statement_reproduces_the_golden_rows(rm_golden):
    """every user as an entry-less resident profile: that user's rows among the reference's 507 triples"""
    model = golden_model(rm_golden)
    users = np.unique(rm_golden["coo"][0]).tolist()
    composed, c = RP.compose(model, [(x, [], [], None) for x in users], "resident")
    assert c["profiles_mine"] == 30 and c["users_unknown"] == c["profiles_empty"] == 0
    groups, rows = RP.score(model, composed, "resident")
    want = {}
    for x, it, sc in rm_golden["recommendations"]:
        want.setdefault(int(x), {})[int(it)] = sc
    assert sum(len(v) for v in want.values()) == 507 and len(rows["rec_user"]) == 507
    assert [g[0] for g in groups] == sorted(want)
    for label, cl, items, scores in groups:
        assert cl == rm_golden["clustering"][label - 1]
        ref = np.array([want[label][int(it)] for it in items])
        assert len(items) == len(want[label])
        assert np.all(np.abs(scores.astype(np.float64) - ref) <= RTOL * np.abs(ref)), label
        assert np.all(np.diff(scores.astype(np.float64)) <= 0)


# users 1 .. 4 in cluster 0, user 9 alone in cluster 1; item 7 is rated by user 9 only, item 8 by nobody kept
HAND = (np.array([1, 1, 1, 2, 2, 3, 3, 3, 4, 9, 9, 4]), np.array([1, 2, 3, 1, 4, 2, 3, 4, 1, 7, 1, 8]),
        np.array([5, 3, 1, 4, 2, 2, 2, 1, 3, 2, 4, 0], dtype=np.float32))
HAND_MAP = (np.array([1, 2, 3, 4, 9]), np.array([0, 0, 0, 0, 1]))


def hand_model(lam=0.5):
    return RP.Model(*HAND, lam, 10, HAND_MAP)


def test_rank_order_and_cluster_items():
    m = hand_model()
    assert m.clusters[0]["items"].tolist() == [1, 2, 3, 4]          # 3 raters, then 2 each by ascending id
    assert m.clusters[1]["items"].tolist() == [1, 7]
    assert m.cluster_of == {1: 0, 2: 0, 3: 0, 4: 0, 9: 1}


def test_every_composition_rule_and_counter():
    m = hand_model()
    profiles = [
        (1, [4, 4, 2, 8, -3, 99], [1.0, 2.0, 0.0, 1.0, 1.0, 1.0], [0, 0, 0, 0, 0, 0]),      # duplicate, a score of 0 on an own item, three unknown
        (2, [1, 2, 3], [0.0, 1.0, float("nan")], [1, 0, 0]),                                # delete own, add, NaN on an absent item
        (3, [1, 1], [3.0, 0.0], [0, 1]),                                                    # write then delete of an absent item
        (77, [1], [1.0], None),                                                             # unknown user
        (1, [], [], None),                                                                  # same label again, unchanged
        (4, [1], [-1.0], None),                                                             # its only item goes: empty
        (9, [7, 2], [1.0, 1.0], [1, 0]),                                                    # item 2 has no column in cluster 1
    ]
    composed, c = RP.compose(m, profiles, "resident", filter_users=0)
    assert composed == [(1, 0, [1, 3, 4]), (2, 0, [2, 4]), (3, 0, [2, 3, 4]), None, (1, 0, [1, 2, 3]), (4, 0, []), (9, 1, [1])]
    assert c == dict(profiles_asked=7, profiles_mine=7, profiles_scored=0, profiles_empty=1, users_unknown=1, users_filtered=0, entries=15,
                     entries_unknown_item=4, entries_nonpositive=3, entries_superseded=2, removes_hit=2, removes_missed=1, items_composed=12)
    # filterUsers, the range of a rank, whole profiles
    composed, c = RP.compose(m, profiles, "resident", filter_users=3)
    assert [x is None for x in composed] == [True, True, False, True, True, False, False] and c["users_filtered"] == 3 and c["users_unknown"] == 1
    assert c["entries"] == 15 and c["entries_unknown_item"] == 1
    parts = [RP.compose(m, profiles, "resident", rank=r, world=3) for r in range(3)]
    assert [p[1]["profiles_mine"] for p in parts] == [2, 2, 3]
    assert sum((p[0] for p in parts), []) == RP.compose(m, profiles, "resident")[0]
    composed, c = RP.compose(m, profiles, "whole", clusters=[0, 0, 0, 1, 0, 0, 1])
    assert composed == [(1, 0, [4]), (2, 0, [2]), (3, 0, []), (77, 1, [1]), (1, 0, []), (4, 0, []), (9, 1, [])]
    assert c["removes_hit"] == 0 and c["removes_missed"] == 3 and c["users_unknown"] == 0 and c["profiles_empty"] == 4


def test_scores_are_the_direct_sums():
    m = hand_model()
    K = m.clusters[0]
    composed, _ = RP.compose(m, [(1, [4, 1], [1.0, 0.0], None), (5, [1, 3], [1.0, 1.0], None)], "resident")
    groups, rows = RP.score(m, composed, "resident")
    assert composed[1] is None and len(groups) == 1
    label, cl, items, scores = groups[0]
    assert set(items.tolist()) == {1} and cl == 0          # profile {2, 3, 4}: item 1, which the prepared row holds, is a candidate again
    C = K["C"][1:]                                           # the neighbours of user 1 (row 0)
    want = 2 * np.log(10.0) - 3 * np.log(4.0) + sum(np.log(float(C[:, 0] @ C[:, j])) for j in (1, 2, 3))
    assert scores[0] == np.float32(want)
    groups, rows = RP.score(m, RP.compose(m, [(5, [1, 3], [1.0, 1.0], None)], "whole", clusters=[0])[0], "whole")
    C = K["C"]
    for it, sc in zip(groups[0][2].tolist(), groups[0][3].tolist()):
        i = K["col"][it]
        assert sc == np.float32(np.log(10.0) - 2 * np.log(5.0) + np.log(float(C[:, i] @ C[:, 0])) + np.log(float(C[:, i] @ C[:, 2])))
    assert rows["rec_user"].tolist() == [0, 0] and rows["rec_cluster"].tolist() == [0, 0]
    # a profile that covers its cluster, the one-user cluster, the only-rater rule at lambda = 0
    assert RP.score(m, RP.compose(m, [(1, [4], [1.0], None)], "resident")[0], "resident")[0] == []
    g = RP.score(m, RP.compose(m, [(9, [7], [1.0], [1])], "resident")[0], "resident")[0]
    assert g[0][2].tolist() == [7] and np.isneginf(g[0][3]).all()
    m0 = hand_model(0.0)
    g = RP.score(m0, RP.compose(m0, [(9, [7], [1.0], None)], "whole", clusters=[1])[0], "whole")[0]
    assert g[0][2].tolist() == [1] and np.isfinite(g[0][3]).all()          # one neighbour, who rated both
    g = RP.score(m0, RP.compose(m0, [(2, [4], [0.0], None)], "resident")[0], "resident")[0]
    lookup = dict(zip(g[0][2].tolist(), g[0][3].tolist()))
    # profile {1}: user 1 rated 1 with 2 and with 3; of the raters of 4 (users 2 and 3) only user 2 itself rated 1
    assert np.isfinite(lookup[2]) and np.isfinite(lookup[3]) and np.isneginf(lookup[4])


def test_header_symbols_and_library_agree():
    P = pkg()
    P.build()
    lib = P._native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "filmyou.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fy_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in P._native.SYMBOLS and hasattr(lib, name), name
    assert "fy_rm2_profiles;" in header and "fy_rm2_profile_stats;" in header
    assert lib.fy_abi_version() == 5      # purely additive


def test_struct_sizes():
    N = pkg()._native
    assert C.sizeof(N.RM2Profiles) == 72 and N.RM2Profiles.cluster.offset == 48 and N.RM2Profiles.base.offset == 56
    assert N.RM2Profiles.world.offset == 64
    assert C.sizeof(N.RM2ProfileStats) == 18 * 8 and all(t is C.c_int64 for _, t in N.RM2ProfileStats._fields_)
    assert [k for k, _ in N.RM2ProfileStats._fields_][:13] == list(RP.COUNTERS)
    assert [k for k, _ in N.RM2ProfileStats._fields_][13:] == [k for k, _ in N.RM2RequestStats._fields_][2:7]
    assert C.sizeof(N.RM2Request) == 16 and C.sizeof(N.RM2RequestStats) == 64 and C.sizeof(N.ItemCFProfiles) == 56


def test_null_arguments_and_packing_without_a_device():
    N = pkg()._native
    lib = N.load()
    prof = N.RM2Profiles(0, None, None, None, None, None, None, 0, 0, 1)
    fake_job = C.c_void_p(8)          # never dereferenced: every call below is refused on its NULL argument first
    for job, q in ((None, C.byref(prof)), (fake_job, None)):
        out = C.c_void_p(1)
        assert lib.fy_rm2_score_profiles(job, q, C.byref(out)) == -1 and not out.value
        assert b"NULL" in lib.fy_last_error()
    assert lib.fy_rm2_score_profiles(None, C.byref(prof), None) == -1 and b"out is NULL" in lib.fy_last_error()
    assert lib.fy_result_rm2_profile_stats(None, C.byref(N.RM2ProfileStats())) == -1 and b"NULL" in lib.fy_last_error()
    mod = importlib.import_module("filmyou-core_amd.host")
    # the sequence form: writes in order, an id outside int32 becomes -1, remove only where a profile has one
    q, keep = mod._rm2_profiles([(4, [1, 2 ** 40, 3], [1.0, 2.0, 3.0]), (5, [], []), (4, [9], [0.5], [1])], "resident", None, 1, 3)
    (labels, start, item, score, remove), cl = keep
    assert q.n_profiles == 3 and q.base == 1 and (q.rank, q.world) == (1, 3) and q.cluster is None and cl is None
    assert labels.tolist() == [4, 5, 4] and start.tolist() == [0, 3, 3, 4] and item.tolist() == [1, -1, 3, 9]
    assert score.tolist() == [1.0, 2.0, 3.0, 0.5] and remove.tolist() == [0, 0, 0, 1]          # scores as given: no shift on this path
    assert (q.user, q.start, q.item, q.score, q.remove) == tuple(a.ctypes.data for a in (labels, start, item, score, remove))
    # the CSR form, one cluster for all and one per profile
    q, keep = mod._rm2_profiles((np.array([7, 8]), [0, 1, 2], [5, 6], [1.0, 2.0]), "whole", 3, 0, 1)
    assert q.n_profiles == 2 and q.base == 0 and q.remove is None and keep[1].tolist() == [3, 3] and keep[1].dtype == np.int32
    assert keep[0][1].dtype == np.int64 and q.cluster == keep[1].ctypes.data
    q, keep = mod._rm2_profiles((np.array([7, 8]), [0, 1, 2], [5, 6], [1.0, 2.0], [0, 1]), "whole", [2, 0], 0, 1)
    assert keep[1].tolist() == [2, 0] and keep[0][4].tolist() == [0, 1]
    with pytest.raises(ValueError, match="clusters"):
        mod._rm2_profiles([(1, [1], [1.0])], "whole", None, 0, 1)
    with pytest.raises(ValueError, match="clusters"):
        mod._rm2_profiles([(1, [1], [1.0]), (2, [1], [1.0])], "whole", [0, 1, 2], 0, 1)
    with pytest.raises(ValueError):
        mod._rm2_profiles([(1, [1, 2], [1.0])], "whole", 0, 0, 1)
    with pytest.raises(ValueError):
        mod._rm2_profiles([(1, [1], [1.0])], "both", 0, 0, 1)
