"""The two row walks of the 24-bit scoring kernels (FY_SCORE_WALK, fy_rm2_kernels.hpp: fy_batch8_p24) give the same bits, and the strided
k_topn_select gives the same rows as the fast top-N.

The second walk differs from the first only in bookkeeping -- the (idx, e, q) triplets of a full batch of eight rows by scalar loads,
the row address in scalar registers, the mask of the user's own items found once per list, packed FMAs -- so every score must come out
bit for bit.  Where it can go wrong is at the ends of lists: a list shorter than a batch, a list of exactly one or two batches, a batch
more or less, the short last batch of a heavy user's quarter, the list that ends the CSR arrays, rated columns on a chunk's first and last
column.  The data below is built by hand around those cases: 900 users, 700 items (three 256-column chunks, the last one partial), one
cluster, half-star ratings.  An item's column is its popularity rank, so the item counts are made to fall with the item id (strictly
at the chunk borders): column = id - 1.
"""
import functools

import numpy as np
import pytest

import oracle
from util import assert_topn_matches, pkg

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, TOP_N = 900, 700, 10
ENV = {"FY_M24_MIN_ITEMS": "0", "FY_PRUNE_MIN_ITEMS": "256", "FY_PRUNE_MIN_USERS": "1", "FY_SEED_CHUNKS": "1", "FY_SCORE_HEAVY": "100"}
LIGHT = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65)
HEAVY = (101, 300, 699)      # 300: quarters of 80 / 80 / 80 / 60 rows, the last wave ends in a short batch
BORDERS = (0, 255, 256, 511, 699)


@functools.lru_cache(maxsize=None)
def dataset(min8):
    """(user, item, score).  min8: every list has at least eight entries and several exactly eight, so the list
    that ends the CSR arrays (slots are in descending order of degree) is one full batch."""
    rng = np.random.default_rng(20261018)
    lists = []                                       # the special users' columns
    for n in LIGHT + HEAVY:
        n = max(n, 8) if min8 else n
        lists.append(np.setdiff1d(np.arange(N_ITEMS), [350]) if n == 699 else np.sort(rng.choice(N_ITEMS, n, replace=False)))
    lists.append(np.arange(256))                     # every column of chunk 0 and nothing else
    lists.append(np.array(sorted(BORDERS + ((100, 300, 600) if min8 else ()))))
    n_special = len(lists)
    special = np.zeros(N_ITEMS, dtype=np.int64)
    for cols in lists:
        special[cols] += 1
    # raters per item: falling with the column, strictly where a test case depends on the exact column
    # (sparse enough for the brute-force oracle and for pairs nobody co-rated; the columns behind the seed chunk far less popular than
    # the seed's, so that the bounds cut most of their blocks and the job does not fall back to the full pass)
    cols = np.arange(N_ITEMS)
    target = np.where(cols < 256, 100 + (255 - cols) * 100 // 255, 10 + (N_ITEMS - 1 - cols) // 32)
    for b in (1, 255, 256, 257, 511, 512, 699):
        if target[b - 1] <= target[b]:
            target[:b] += 1
    fill = target - special
    assert fill.min() >= 0
    # the other users: a large group with short lists and a small one with long lists, each user with a weight of its own
    group_b = np.arange(n_special, n_special + 104)
    group_a = np.arange(n_special + 104, N_USERS)
    w_a, w_b = rng.uniform(0.7, 1.6, len(group_a)), rng.uniform(0.5, 1.5, len(group_b))
    per_user = [list(c) for c in lists] + [[] for _ in range(N_USERS - n_special)]
    for j in range(N_ITEMS):
        nb = int(round(fill[j] * 0.45))
        for u in rng.choice(group_b, nb, replace=False, p=w_b / w_b.sum()):
            per_user[u].append(j)
        for u in rng.choice(group_a, int(fill[j]) - nb, replace=False, p=w_a / w_a.sum()):
            per_user[u].append(j)
    user = np.concatenate([np.full(len(c), u + 1, dtype=np.int32) for u, c in enumerate(per_user)])
    col = np.concatenate([np.asarray(c, dtype=np.int32) for c in per_user])
    score = (0.5 * (1 + (user.astype(np.int64) * 7 + col.astype(np.int64) * 13) % 10)).astype(np.float32)
    counts = np.bincount(col, minlength=N_ITEMS)
    assert np.array_equal(counts, target) and np.all(np.diff(counts) <= 0)
    assert all(counts[b - 1] > counts[b] for b in (1, 255, 256, 257, 511, 512, 699))
    lengths = np.bincount(user)[1:]
    assert lengths.min() == (8 if min8 else 1) and (lengths == 8).sum() >= (4 if min8 else 1)
    assert (lengths <= 100).sum() >= 200 and (lengths > 100).sum() >= 50      # light users and heavy ones (FY_SCORE_HEAVY=100)
    return user, (col + 1).astype(np.int32), score


@functools.lru_cache(maxsize=None)
def reference(min8, lam):
    u, i, s = dataset(min8)
    uu = np.unique(u)
    return oracle.rm2(u, i, s, lam=float(lam), number_of_items=N_ITEMS, number_of_recommendations=1 << 30, number_of_clusters=1,
                      map_user=uu, map_cluster=np.zeros(len(uu), dtype=np.int32), n_threads=8)


def run_job(monkeypatch, min8, lam, env):
    """One job in a context of its own (the library reads FY_* when the context is created).  Returns copies: rows, side outputs, stats."""
    P = pkg()
    for k, v in {**ENV, **env}.items():
        monkeypatch.setenv(k, v)
    u, i, s = dataset(min8)
    uu = np.unique(u)
    conf = P.Configuration()
    conf.set("lambda", lam)
    conf.setInt("numberOfItems", N_ITEMS)
    conf.setInt("numberOfClusters", 1)
    conf.setInt("numberOfRecommendations", TOP_N)
    ctx = P.Context(0)
    rec = P.RM2Job(conf, ctx).run((u, i, s), clustering=(uu, np.zeros(len(uu), dtype=np.int32)))
    rows = {k: np.array(v, copy=True) for k, v in rec.rows().items()}
    sums = {k: np.array(v, copy=True) for k, v in rec.sums().items()}
    stats = dict(rec.stats)
    rec.close()
    ctx.close()
    return rows, sums, stats


def assert_same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), k


FLOWS = {"default": {}, "fused_bounds": {"FY_SUP_BOUNDS": "0"}, "full_pass": {"FY_PRUNE": "0"}}


def check_walks(monkeypatch, min8, lam, flow):
    r0, s0, st0 = run_job(monkeypatch, min8, lam, {**FLOWS[flow], "FY_SCORE_WALK": "0"})
    r1, s1, st1 = run_job(monkeypatch, min8, lam, {**FLOWS[flow], "FY_SCORE_WALK": "1"})
    assert_same_bytes(r0, r1)          # (a) user, item, score bits, cluster
    assert_same_bytes(s0, s1)          #     and the side outputs
    for st in (st0, st1):
        if flow == "full_pass":
            assert st["blocks_total"] == 0
        else:
            assert st["blocks_total"] > 0, "the branch and bound did not run"
            # (lambda = 0: most seed lists end in -inf, tau is -inf, no block can be excluded and the batch takes the full pass instead)
            if lam != "0.0":
                assert st["prune_fallbacks"] == 0
                if flow == "default":
                    assert st["blocks_survived"] > 0, "no block survived: k_score_blocks did not run"
    assert st0["log_terms_evaluated"] == st1["log_terms_evaluated"]
    assert_topn_matches(r1, reference(min8, lam), TOP_N)      # (b) the tolerance of every forced 24-bit job: relative 1e-5
    return r1


@pytest.mark.parametrize("lam", ["0.1", "0.0"])
@pytest.mark.parametrize("flow", list(FLOWS))
def test_both_walks_give_the_same_bits(monkeypatch, flow, lam):
    """lambda = 0: a never co-rated pair is a zero term, the score -inf (quirk Q7): those rows stay, in both walks."""
    ref = reference(False, lam)
    if lam == "0.0":
        assert np.isneginf(ref["rec_score"]).any(), "the data has no never co-rated pair"
    rows = check_walks(monkeypatch, False, lam, flow)
    if lam == "0.0":
        assert np.isneginf(rows["score"]).any()


def test_the_list_that_ends_the_arrays_is_a_full_batch(monkeypatch):
    check_walks(monkeypatch, True, "0.1", "default")


@pytest.mark.parametrize("lam", ["0.1", "0.0"])
@pytest.mark.parametrize("flow", ["default", "full_pass"])
def test_strided_select_equals_fast_topn(monkeypatch, flow, lam):
    """(c) k_topn_select runs at most two workgroups per CU and strides over the users: 900 users are more than that.  In the full pass
    FY_TOPN_FORCE_SELECT=1 sends every user through it (in the pruned flow only those whose seed list does not stand)."""
    fast, _, st_fast = run_job(monkeypatch, False, lam, {**FLOWS[flow], "FY_TOPN_FORCE_SELECT": "0"})
    sel, _, st_sel = run_job(monkeypatch, False, lam, {**FLOWS[flow], "FY_TOPN_FORCE_SELECT": "1"})
    assert st_sel["topn_select_users"] > st_fast["topn_select_users"]
    if flow == "full_pass":
        assert st_sel["topn_select_users"] == len(np.unique(sel["user"])) > 512
    assert_same_bytes(fast, sel)
