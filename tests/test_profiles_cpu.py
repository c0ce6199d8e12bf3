"""Lists for given profiles: the new ABI symbols and struct layouts, the refusals that need no device, and the plain statement
(tests/profile_ref.py) against the two statements it must agree with -- composition against tests/ratings_update_ref.py applied to
single-user ratings, lists of a resident row against tests/estimate_ref.py's kept preferences and cells.  No GPU."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import estimate_ref as ER
import oracle
import profile_ref as PR
import ratings_update_ref as UR
from util import pkg

NEW = ("fy_itemcf_recommend_profiles", "fy_result_itemcf_profile_stats")


def test_header_and_library_agree_on_the_new_symbols():
    P = pkg()
    P.build()
    lib = P._native.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "filmyou.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(fy_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in P._native.SYMBOLS and hasattr(lib, name), name
    assert "FY_PROFILE_WHOLE = 0" in header and "FY_PROFILE_ON_RESIDENT = 1" in header
    assert lib.fy_abi_version() == 5          # additive: the old ABI is untouched


def test_struct_sizes():
    N = pkg()._native
    assert C.sizeof(N.ItemCFProfiles) == 56 and N.ItemCFProfiles.start.offset == 16 and N.ItemCFProfiles.base.offset == 48
    assert C.sizeof(N.ItemCFProfileStats) == 17 * 8 and all(t is C.c_int64 for _, t in N.ItemCFProfileStats._fields_)
    assert N.ItemCFProfileStats.items_needed.offset == 88 and N.ItemCFProfileStats.batches.offset == 128
    assert [k for k, _ in N.ItemCFProfileStats._fields_][11:] == [k for k, _ in N.ItemCFRequestStats._fields_][2:]      # the six row-store fields
    assert (N.FY_PROFILE_WHOLE, N.FY_PROFILE_ON_RESIDENT) == (0, 1)
    assert C.sizeof(N.ItemCFParams) == 24 and C.sizeof(N.ItemCFFilter) == 40 and C.sizeof(N.ItemCFRequestStats) == 64


def test_null_arguments_without_a_device():
    N = pkg()._native
    lib = N.load()
    prm = N.ItemCFParams(10, 50, 0, 0, 1, 0)
    prof = N.ItemCFProfiles(0, None, None, None, None, None, 0)
    fake_job = C.c_void_p(8)          # never dereferenced: every call below is refused on its NULL argument first
    for job, p, q in ((None, C.byref(prm), C.byref(prof)), (fake_job, None, C.byref(prof)), (fake_job, C.byref(prm), None)):
        out = C.c_void_p(1)
        assert lib.fy_itemcf_recommend_profiles(job, p, q, None, C.byref(out)) == -1 and not out.value
        assert b"NULL" in lib.fy_last_error()
    assert lib.fy_itemcf_recommend_profiles(None, C.byref(prm), C.byref(prof), None, None) == -1 and b"out is NULL" in lib.fy_last_error()
    assert lib.fy_result_itemcf_profile_stats(None, C.byref(N.ItemCFProfileStats())) == -1 and b"NULL" in lib.fy_last_error()
    # the Python layer refuses what it can before the library sees it
    mod = importlib.import_module("filmyou-core_amd.host")
    with pytest.raises(ValueError):
        mod._itemcf_profiles([(1, [1, 2], [1.0])], "whole", 0.0)
    with pytest.raises(ValueError):
        mod._itemcf_profiles([(1, [1], [1.0])], "both", 0.0)
    q, keep = mod._itemcf_profiles([(4, [1, 2 ** 40, 3], [1.0, 2.0, 3.0]), (5, [], []), (4, [9], [0.5], [1])], "resident", 0.25)
    assert q.n_profiles == 3 and q.base == 1 and keep[1].tolist() == [0, 3, 3, 4] and keep[2].tolist() == [1, -1, 3, 9]
    assert keep[3].tolist() == [1.25, 2.25, 3.25, 0.75] and keep[4].tolist() == [0, 0, 0, 1]
    q, keep = mod._itemcf_profiles((np.array([7, 8]), [0, 1, 2], [5, 6], [1.0, 2.0]), "whole", 0.0)
    assert q.n_profiles == 2 and q.base == 0 and q.remove is None and keep[1].dtype == np.int64


def catalogue(rng):
    """ratings of other users over items 1 .. 12 (item 5 and item 11 rated by nobody), popularity with ties"""
    items = np.array([1, 2, 3, 4, 6, 7, 8, 9, 10, 12], dtype=np.int32)
    u, i = [], []
    for x in range(100, 100 + int(rng.integers(3, 9))):
        pick = rng.choice(items, size=int(rng.integers(1, len(items) + 1)), replace=False)
        u += [x] * len(pick)
        i += pick.tolist()
    missing = np.setdiff1d(items, np.array(i))
    u += [99] * len(missing)          # every catalogue item has a rater
    i += missing.tolist()
    s = rng.integers(1, 11, size=len(u)) / 2.0
    return np.array(u, dtype=np.int32), np.array(i, dtype=np.int32), s.astype(np.float32)


def test_composition_is_the_ratings_tables_write_semantics():
    rng = np.random.default_rng(2024)
    seen = dict(dup=0, del_absent=0, del_then_write=0, unknown=0, empty=0)
    for case in range(200):
        u, i, s = catalogue(rng)
        known = set(i.tolist())
        base = "resident" if case % 2 else "whole"
        if base == "resident" and case % 8 != 1:          # (case % 8 == 1: a user the job does not know)
            row_items = rng.choice(np.array(sorted(known)), size=int(rng.integers(1, 7)), replace=False).astype(np.int32)
            row_scores = (rng.integers(1, 11, size=len(row_items)) / 2.0).astype(np.float32)
            u = np.concatenate([u, np.full(len(row_items), 1, dtype=np.int32)])
            i = np.concatenate([i, row_items])
            s = np.concatenate([s, row_scores])
        else:
            row_items, row_scores = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)
        n = int(rng.integers(0, 12))
        items = rng.choice(np.array([1, 2, 3, 4, 5, 6, 7, 8, 11, -2]), size=n).astype(np.int32)          # few items: duplicates are the rule
        scores = (rng.integers(1, 11, size=n) / 2.0).astype(np.float32)
        remove = (rng.random(n) < 0.35).astype(np.uint8)
        composed, c = PR.compose(u, i, s, [(1, items.tolist(), scores.tolist(), remove.tolist())], base)
        # the same through the ratings table's statement: unknown items never reach the table
        has_col = np.array([int(x) in known for x in items], dtype=bool) if n else np.zeros(0, dtype=bool)
        src = (row_items, row_scores) if base == "resident" else (row_items[:0], row_scores[:0])
        ou, oi, os_, uc = UR.apply_writes(np.full(len(src[0]), 1), src[0], src[1], np.full(int(has_col.sum()), 1), items[has_col], scores[has_col],
                                          remove[has_col])
        rank = PR.popularity_rank(i)
        want = sorted(zip(oi.tolist(), os_.tolist()), key=lambda kv: rank[kv[0]])
        assert composed == [(1, want)], (case, composed, want)
        assert [rank[it] for it, _ in composed[0][1]] == sorted(rank[it] for it, _ in composed[0][1])
        assert c["entries"] == n and c["entries_unknown_item"] == n - int(has_col.sum())
        assert c["entries_superseded"] == uc["n_superseded"] and c["removes_hit"] == uc["n_deleted"] and c["removes_missed"] == uc["n_delete_missed"]
        assert c["prefs_composed"] == uc["nnz_out"] == len(want) and c["profiles_empty"] == (not want)
        assert c["users_unknown"] == (base == "resident" and len(row_items) == 0)
        # the cases the statement must have met
        cols = items[has_col].tolist()
        seen["dup"] += len(set(cols)) < len(cols)
        seen["del_absent"] += uc["n_delete_missed"] > 0
        seen["unknown"] += c["entries_unknown_item"] > 0
        seen["empty"] += not want
        rm = remove[has_col].tolist()
        seen["del_then_write"] += any(rm[a] and not rm[b] and cols[a] == cols[b] for a in range(len(cols)) for b in range(a + 1, len(cols)))
    print(seen)
    assert all(v >= 10 for v in seen.values()), seen


def golden(rm_golden):
    u, i, s = rm_golden["coo"]
    keep = (s > 0) & (u != 7) & (i != 13)
    return u[keep], i[keep], s[keep]


@pytest.mark.parametrize("boolean", [False, True])
@pytest.mark.parametrize("max_prefs,K", [(8, 20), (50, 10)])
def test_lists_of_a_resident_row_are_the_estimate_statements_cells(rm_golden, max_prefs, K, boolean):
    u, i, s = golden(rm_golden)
    sims = oracle.itemsim(u, i, s, max_similarities_per_item=K)
    users = np.unique(u).tolist()
    composed, c = PR.compose(u, i, s, [(x, [], [], None) for x in users], "resident")
    assert c["prefs_composed"] == len(u) and c["users_unknown"] == 0 and c["profiles_empty"] == 0
    got = PR.lists(composed, sims["item"], sims["other"], sims["sim"], max_prefs, boolean)
    kept = ER.kept_preferences(u, i, s, max_prefs)
    rows = ER.similarity_rows(sims["item"], sims["other"], sims["sim"])
    want = []
    for x in users:
        assert PR.kept(dict(composed)[x], max_prefs) == kept[x]          # the same preferences in the same order
        cells, own = ER.user_cells(kept[x], rows, boolean)
        mine = []
        for it, (num, den, cnt) in cells.items():
            if it in own or cnt < (1 if boolean else 2) or num == 0.0:
                continue
            v = float(np.float32(num if boolean else num / den))
            if not math.isnan(v):
                mine.append((x, it, v))
        want += sorted(mine, key=lambda t: -t[2])
    assert len(want) > 100
    assert list(zip(got["user"].tolist(), got["item"].tolist(), got["score"].tolist())) == want
    # and the oracle of item-based CF says the same
    ref = oracle.itemcf(u, i, s, sims["item"], sims["other"], sims["sim"], num_recommendations=1 << 30, max_prefs_per_user=max_prefs, boolean_data=boolean)
    assert set(zip(ref["user"].tolist(), ref["item"].tolist())) == {(a, b) for a, b, _ in want}
