"""Deterministic inputs for the factorisation and refinement tests at the kernels' chunk, grid and k limits (test_nmf_gpu.py,
test_refine_gpu.py, test_factor_edge_inputs_cpu.py).  Plain numpy, no GPU.  Every builder asserts the properties its tests depend
on and obeys the reference's preconditions: every user rates something, every item is rated, no (user, item) twice.  The numbers
the lengths are built around (NMF_CHUNK = 512, RF_CHUNK = 256, the 4096-workgroup caps) are read back from the sources by
test_factor_edge_inputs_cpu.py, so that a changed constant cannot turn these shapes into small ones unnoticed."""
import functools

import numpy as np

import refine_ref as RR

HUB_USER_LENGTHS = (511, 512, 513, 1023, 1024, 1025, 1026, 1027)      # around one and two chunks of 512; 1024..1027: tails 0..3 of the 4-way walk
HUB_ITEM_LENGTHS = (513, 514, 515, 1025, 1200)

WRAP_USERS, WRAP_ITEMS, WRAP_PER_USER = 17000, 300, 62
TALL_USERS, TALL_ITEMS, TALL_K = 1048576 + 5, 40, 2

PARENT_USERS = (600, 40, 2)                 # with usersPerSubCluster = 8: k = 75, 5, 1; with 120: k = 5, 1, 1
PARENT_ITEMS = (800, 600, 5)                # disjoint item ranges, one per parent
PARENT_A_USER_LENGTHS = (700,)
PARENT_A_ITEM_LENGTHS = (600, 257, 515)     # 256 + 256 + 88; one entry beyond a chunk; two chunks and a tail of three
PARENT_B_USER_LENGTHS = (255, 256, 257, 258, 511, 513)     # tails 3, 0, 1, 2 of the four-way walk at a chunk end


def worst_relative(got, want):
    """The largest relative error, for the figures the tests print in front of their assertions."""
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))) if want.size else 0.0


def half_stars(user, item):
    """0.5 .. 5.0 as a fixed function of the pair"""
    return (0.5 * (1 + (np.asarray(user, np.int64) * 7 + np.asarray(item, np.int64) * 13) % 10)).astype(np.float32)


def _fill_rows(M, rows, lengths, free_cols, rng):
    """Row r gets ratings on random free columns until it holds exactly its length."""
    for r, n in zip(rows, lengths):
        need = n - int(M[r].sum())
        assert 0 <= need <= len(free_cols)
        M[r, rng.choice(free_cols, need, replace=False)] = True


def _background(M, rows, cols, density, rng):
    """Random ratings on rows x cols; every such row and column ends with at least one."""
    block = rng.random((len(rows), len(cols))) < density
    block[np.arange(len(rows)), rng.integers(0, len(cols), len(rows))] = True
    block[rng.integers(0, len(rows), len(cols)), np.arange(len(cols))] = True
    M[np.ix_(rows, cols)] = block


def _coo(M, rng, n_dropped=2):
    """The matrix's pairs as 1-based COO with half-star scores, plus dropped entries (score 0.0 and -1.0) on pairs the matrix does
    not hold, in a random order."""
    u, i = np.nonzero(M)
    au, ai = np.nonzero(~M)
    pick = rng.choice(len(au), n_dropped, replace=False)
    user, item = np.r_[u, au[pick]] + 1, np.r_[i, ai[pick]] + 1
    score = np.r_[half_stars(u + 1, i + 1), np.float32([0.0, -1.0])[:n_dropped]]
    order = rng.permutation(len(user))
    return user[order].astype(np.int32), item[order].astype(np.int32), score[order].astype(np.float32)


def _assert_no_duplicates(user, item):
    assert len(np.unique(user.astype(np.int64) << 32 | item.astype(np.int64))) == len(user)


@functools.lru_cache(maxsize=None)
def hubs():
    """1300 users x 1100 items at about 1 % density, with hub users of exactly HUB_USER_LENGTHS kept ratings and hub items of exactly
    HUB_ITEM_LENGTHS raters.  Returns a dict: coo, n_users, n_items, hub_users / hub_items (1-based ids, in the order of the length
    tuples).  Every hub user rates every hub item, so both kinds of length are fixed by the other ids alone."""
    rng = np.random.default_rng(20261019)
    n_users, n_items = 1300, 1100
    hub_u = np.sort(rng.choice(n_users, len(HUB_USER_LENGTHS), replace=False))
    hub_i = np.sort(rng.choice(n_items, len(HUB_ITEM_LENGTHS), replace=False))
    plain_u, plain_i = np.setdiff1d(np.arange(n_users), hub_u), np.setdiff1d(np.arange(n_items), hub_i)
    M = np.zeros((n_users, n_items), bool)
    _background(M, plain_u, plain_i, 0.01, rng)
    M[np.ix_(hub_u, hub_i)] = True
    _fill_rows(M, hub_u, HUB_USER_LENGTHS, plain_i, rng)
    Mt = M.T.copy()
    _fill_rows(Mt, hub_i, HUB_ITEM_LENGTHS, plain_u, rng)
    M = Mt.T.copy()
    user, item, score = _coo(M, rng)
    kept = score > 0
    _assert_no_duplicates(user, item)
    assert (~kept).sum() == 2 and set(np.unique(score[kept]).tolist()) == set((0.5 * np.arange(1, 11)).tolist())
    ulen, ilen = np.bincount(user[kept], minlength=n_users + 1)[1:], np.bincount(item[kept], minlength=n_items + 1)[1:]
    assert ulen[hub_u].tolist() == list(HUB_USER_LENGTHS) and ilen[hub_i].tolist() == list(HUB_ITEM_LENGTHS)
    assert ulen.min() >= 1 and ilen.min() >= 1
    assert ulen[plain_u].max() < 100 and ilen[plain_i].max() < 100          # the hubs are the only long rows
    background = kept.sum() - ulen[hub_u].sum() - ilen[hub_i].sum() + len(hub_u) * len(hub_i)      # the hub x hub block is in both sums
    assert 0.005 < background / (len(plain_u) * len(plain_i)) < 0.02
    assert not np.array_equal(user, np.sort(user))                          # shuffled COO
    return {"coo": (user, item, score), "n_users": n_users, "n_items": n_items, "hub_users": hub_u + 1, "hub_items": hub_i + 1,
            "user_lengths": ulen, "item_lengths": ilen}


@functools.lru_cache(maxsize=None)
def wrap():
    """17 000 users x 300 items, 62 distinct items per user: more ratings than 4096 x 256 threads, more users (one chunk each) than
    4096 x 4 waves, every item in several chunks.  With k = 64 the loops that go round more than once are those over the ratings
    (k_nmf_keys), over the chunks and rows by wave (k_nmf_spmm_chunks, k_nmf_update) and over the elements of H
    (k_nmf_spmm_reduce).  The thread-per-row table builders do not wrap below 1 048 576 rows: tall() is for them."""
    rng = np.random.default_rng(20261020)
    cols = np.argsort(rng.random((WRAP_USERS, WRAP_ITEMS)), axis=1)[:, :WRAP_PER_USER]
    user = np.repeat(np.arange(1, WRAP_USERS + 1), WRAP_PER_USER)
    item = cols.ravel() + 1
    order = rng.permutation(len(user))
    user, item = user[order].astype(np.int32), item[order].astype(np.int32)
    score = half_stars(user, item)
    _assert_no_duplicates(user, item)
    ilen = np.bincount(item, minlength=WRAP_ITEMS + 1)[1:]
    assert len(user) == 1054000 > 1048576 and WRAP_USERS > 16384 and WRAP_USERS * 64 > 1048576
    assert np.all(np.bincount(user)[1:] == WRAP_PER_USER) and ilen.min() > 512
    return {"coo": (user, item, score), "n_users": WRAP_USERS, "n_items": WRAP_ITEMS, "item_lengths": ilen}


@functools.lru_cache(maxsize=None)
def tall():
    """1 048 581 users x 40 items, two distinct items per user: more user rows than 4096 x 256 threads, so the thread-per-row
    loops that build the CSR and chunk tables (k_nmf_rowptr, k_nmf_check_rows, k_nmf_chunk_counts, k_nmf_chunk_rows) go round
    more than once on the user side.  (k_nmf_gram_sum strides over k x k <= 65 536 elements and cannot wrap at any allowed k.)"""
    n_users, n_items = TALL_USERS, TALL_ITEMS
    u = np.arange(n_users, dtype=np.int64)
    first = u * 7 % n_items
    second = (first + 1 + u % (n_items - 1)) % n_items           # never the first again
    user = np.r_[u, u] + 1
    item = np.r_[first, second] + 1
    order = np.random.default_rng(20261022).permutation(len(user))
    user, item = user[order].astype(np.int32), item[order].astype(np.int32)
    score = half_stars(user, item)
    _assert_no_duplicates(user, item)
    assert n_users > 1048576 and np.all(np.bincount(user)[1:] == 2) and np.bincount(item, minlength=n_items + 1)[1:].min() > 512
    return {"coo": (user, item, score), "n_users": n_users, "n_items": n_items}


@functools.lru_cache(maxsize=None)
def parents():
    """One COO with three parent clusters of PARENT_USERS users over disjoint item ranges of PARENT_ITEMS ids:

      parent 0   600 users.  One item rated by all of them, one by 257, one by 515, one user with 700 ratings.
      parent 1   40 users, six of them with 255, 256, 257, 258, 511 and 513 ratings.
      parent 2   two users.

    usersPerSubCluster = 8 gives k = 75 (the k > 64 branch), 5 (L = 8: eight rows per wave) and 1.  An item row inside a parent
    cannot be longer than the parent has users and k <= 64 with 8 users per sub-cluster allows 512 users at the most, so the
    long item rows of the k <= 64 branch come from the same input with usersPerSubCluster = 120: k = 5, 1, 1.
    Returns a dict: coo, map_user, map_cluster, K, n_users, and per parent the row lengths AFTER the mapping."""
    rng = np.random.default_rng(20261021)
    n_users, n_items = sum(PARENT_USERS), sum(PARENT_ITEMS)
    M = np.zeros((n_users, n_items), bool)
    raw = rng.permutation(n_users)                         # matrix row -> raw user id - 1: the parents' users are interleaved
    u0, i0 = np.r_[0, np.cumsum(PARENT_USERS)], np.r_[0, np.cumsum(PARENT_ITEMS)]
    # parent 0
    rows, cols = np.arange(u0[0], u0[1]), np.arange(i0[0], i0[1])
    hub_r, hub_c = rows[:1], cols[:3]
    _background(M, rows[1:], cols[3:], 0.015, rng)
    M[np.ix_(hub_r, hub_c)] = True
    _fill_rows(M, hub_r, PARENT_A_USER_LENGTHS, cols[3:], rng)
    Mt = M.T.copy()
    _fill_rows(Mt, hub_c, PARENT_A_ITEM_LENGTHS, rows[1:], rng)
    M = Mt.T.copy()
    # parent 1
    rows, cols = np.arange(u0[1], u0[2]), np.arange(i0[1], i0[2])
    _background(M, rows[6:], cols, 0.02, rng)
    _fill_rows(M, rows[:6], PARENT_B_USER_LENGTHS, cols, rng)
    # parent 2
    M[u0[2]:u0[3], i0[2]:i0[3]] = [[1, 1, 0, 1, 0], [0, 1, 1, 0, 1]]
    mu, mi = np.nonzero(M)
    au, ai = np.nonzero(~M[u0[0]:u0[1], i0[0]:i0[1]])      # the dropped entries: pairs inside parent 0 that nobody rated
    pick = rng.choice(len(au), 2, replace=False)
    user, item = np.r_[raw[mu], raw[au[pick]]] + 1, np.r_[mi, ai[pick]] + 1
    score = np.r_[half_stars(raw[mu] + 1, mi + 1), np.float32([0.0, -1.0])]
    order = rng.permutation(len(user))
    user, item, score = user[order].astype(np.int32), item[order].astype(np.int32), score[order].astype(np.float32)
    _assert_no_duplicates(user, item)
    map_user = (raw + 1).astype(np.int32)
    map_cluster = np.repeat(np.arange(3), PARENT_USERS).astype(np.int32)
    shuffle = rng.permutation(n_users)
    map_user, map_cluster = map_user[shuffle], map_cluster[shuffle]
    # the lengths per parent, after the mapping
    m = RR.mappings(user, item, score, map_user, map_cluster, 3)
    assert [len(x) for x in m["users"]] == list(PARENT_USERS) and [len(x) for x in m["items"]] == list(PARENT_ITEMS)
    assert RR.sub_clusters(m, 8) == [75, 5, 1] and RR.sub_clusters(m, 120) == [5, 1, 1]
    lengths = []
    for c in range(3):
        su, si, _ = RR.extract(user, item, score, m, c)
        ulen, ilen = np.bincount(su, minlength=PARENT_USERS[c] + 1)[1:], np.bincount(si, minlength=PARENT_ITEMS[c] + 1)[1:]
        assert ulen.min() >= 1 and ilen.min() >= 1
        lengths.append((ulen, ilen))
    (ua, ia), (ub, ib), (uc, ic) = lengths
    assert sorted(ua[ua > 100].tolist()) == list(PARENT_A_USER_LENGTHS) and sorted(ia[ia > 100].tolist()) == sorted(PARENT_A_ITEM_LENGTHS)
    assert sorted(ub[ub > 100].tolist()) == list(PARENT_B_USER_LENGTHS) and ib.max() <= PARENT_USERS[1]
    assert uc.tolist() == [3, 3] and ic.tolist() == [1, 2, 1, 1, 1]
    return {"coo": (user, item, score), "map_user": map_user, "map_cluster": map_cluster, "K": 3, "n_users": n_users,
            "lengths": lengths}


def wrap_as_one_parent():
    """wrap() with every user in parent cluster 0."""
    d = wrap()
    users = np.arange(1, d["n_users"] + 1, dtype=np.int32)
    return d["coo"], users, np.zeros(len(users), np.int32)


# ---------------------------------------------------------------- the infinity clamps
def huge_initial(rng, shape):
    """Values around 1e200: their products overflow, their sums with the ratings do not.  (Not 1e150: its second iteration
    lands next to DBL_MAX, where the order of a sum could decide between finite and infinite.)"""
    return (rng.random(shape) + 0.5) * 1e200


def unclamped_ppc_row(u, i, s, H0, W0, j):
    """PPCHComputationReducer's formula for user j + 1 without the infinity clamps, one iteration."""
    with np.errstate(over="ignore", invalid="ignore"):
        sel = (u == j + 1) & (s > 0)
        x = (s[sel].astype(np.float64)[:, None] * W0[i[sel] - 1]).sum(0)
        y = (W0.T @ W0) @ H0[j]
        d, e = H0[j] @ y, H0[j] @ x
        return H0[j] * ((x + d) / ((y + e) + 1e-12))


# ---------------------------------------------------------------- shapes and k values the tests share with the CPU check
K_EDGES = (63, 64, 128, 129, 192, 193, 256)     # around every 64 columns of the register arrays, up to the limit
K_BEYOND = 257                                  # FY_ERR_UNSUPPORTED
K_EDGE_SHAPE = (257, 130)                       # users x items
WRAP_K = 64
WRAP_USERS_PER_SUB_CLUSTER = 400                # one parent of 17 000 users: k = 43, L = 64, one row per wave
ASSIGN_WIDE_ROWS = 16385 + 3
ASSIGN_THREAD_ROWS = 1048576 + 5
