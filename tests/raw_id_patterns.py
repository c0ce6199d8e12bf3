"""Order-preserving relabellings of the raw user and item ids (pure numpy).

Every structure the library builds depends on the raw ids through their ORDER alone: the dense user index is the rank of the raw id, ties in
popularity and in a list break by ascending raw id, side outputs come out in ascending raw id.  So a job run on (f(u), g(i), s) for
strictly increasing f, g -- f mapped over the clustering map and every request list as well -- must give, mapped back through the inverses,
the bytes of the job on the dense ids.  What changes with the MAGNITUDE of the ids is the code this file aims at: the field widths of the
sort keys, the gate of the packed sort mode, the route of the clustering map, the refinement pass's raw-id table, the sharded prep.

patterns(n_users, n_items, n_map) returns {name: (f, g)}; f[k] is the raw id of dense user k + 1 (dense ids are 1-based), g likewise for
items.  The constants each pattern sits on are the library's as they stand in the source; tests/test_raw_id_patterns_cpu.py states every
gate's inequality, so a change of a constant there moves the pattern with it.
"""
import numpy as np

INT32_MAX = 2 ** 31 - 1
# fy_prep.hip, build_structure: host table when `nRU <= 8 * n_map + (1 << 20)`, nRU = max_user + 1
ROUTING_TABLE_SLACK = 1 << 20
ROUTING_TABLE_FACTOR = 8
# fy_rm2.hip, C.refine: `J->S->max_item < (1 << 28)`
REFINE_MAX_ITEM = 1 << 28
# fy_prep.hip, shard_ratings_by_cluster: `nRU + nRI > ((int64_t)1 << 25)` falls back to the replicated prep
SHARD_MAX_RAW_IDS = 1 << 25
NETFLIX_MAX_USER, ML25M_MAX_ITEM = 2649429, 209171


def bits_for(v):
    """fy_prep.hip, build_structure: `bits_for` -- the bits that hold every value <= v."""
    return int(v).bit_length()


def key_bits(max_user, max_item, K):
    """(ib0, ub0, kb0) of fy_prep.hip, build_structure."""
    return max(1, bits_for(max(0, max_item))), max(1, bits_for(max_user + 1)), bits_for(max(0, K - 1))


def packed_gate(max_user, max_item, K):
    """fy_prep.hip, build_structure: `ib0 + ub0 + 16 <= 64 && kb0 + ib0 + ub0 + 16 <= 64` (beside FY_PREP_PACKED and half-exact scores)."""
    ib0, ub0, kb0 = key_bits(max_user, max_item, K)
    return ib0 + ub0 + 16 <= 64 and kb0 + ib0 + ub0 + 16 <= 64


def routing_by_table(max_user, n_map):
    """fy_prep.hip, build_structure: `n_map > 0 && nRU <= 8 * n_map + (1 << 20)`."""
    return n_map > 0 and max_user + 1 <= ROUTING_TABLE_FACTOR * n_map + ROUTING_TABLE_SLACK


def refinement_allowed(max_item):
    """fy_rm2.hip, C.refine: `max_item >= 0 && max_item < (1 << 28)` (beside the flow's own conditions)."""
    return 0 <= max_item < REFINE_MAX_ITEM


def sharded_prep_allowed(max_user, max_item):
    """fy_prep.hip, shard_ratings_by_cluster: not `nRU + nRI > 2^25`."""
    return (max_user + 1) + (max_item + 1) <= SHARD_MAX_RAW_IDS


def dense(n, first=1):
    return np.arange(first, first + n, dtype=np.int64)


def dense_to(n, top):
    """1 .. n - 1 and `top`: dense ids with one outlier that sets the maximum."""
    assert top >= n
    out = dense(n)
    out[-1] = top
    return out


def spread(n, lo, hi):
    """n strictly increasing ids from lo to hi, both included: consecutive at the low end, ever sparser towards hi (a quadratic ramp), so
    neighbours differ in the lowest bit at one end and in the highest at the other."""
    assert n >= 2 and hi - lo >= n - 1
    room = hi - lo - (n - 1)
    out = np.array([lo + k + (room * k * k) // ((n - 1) * (n - 1)) for k in range(n)], dtype=np.int64)
    assert out[0] == lo and out[-1] == hi
    return out


def patterns(n_users, n_items, n_map):
    U, I = n_users, n_items
    edge = ROUTING_TABLE_FACTOR * n_map + ROUTING_TABLE_SLACK        # max_user + 1 at the routing gate
    p = {
        "dense": (dense(U), dense(I)),
        "zero_based": (dense(U, 0), dense(I, 0)),
        "netflix_like": (spread(U, 6, NETFLIX_MAX_USER), spread(I, 1, ML25M_MAX_ITEM)),
        "routing_edge_table": (dense_to(U, edge - 1), dense(I)),
        "routing_edge_sort": (dense_to(U, edge), dense(I)),
        "pack_edge_64": (spread(U, 1, 2 ** 24 - 2), spread(I, 1, 2 ** 24 - 1)),
        "pack_edge_65": (spread(U, 1, 2 ** 24 - 1), spread(I, 1, 2 ** 24 - 1)),
        "pack_edge_k_64": (spread(U, 1, 2 ** 23 - 2), spread(I, 1, 2 ** 24 - 1)),
        "pack_edge_k_65": (spread(U, 1, 2 ** 23 - 1), spread(I, 1, 2 ** 24 - 1)),
        "pow2_item_lo": (dense(U), dense_to(I, 2 ** 16 - 1)),
        "pow2_item_hi": (dense(U), dense_to(I, 2 ** 16)),
        "refine_edge_on": (dense(U), dense_to(I, REFINE_MAX_ITEM - 1)),
        "refine_edge_off": (dense(U), dense_to(I, REFINE_MAX_ITEM)),
        "int32_edge": (spread(U, 0, INT32_MAX), spread(I, 0, INT32_MAX)),
        # user id 2^31 - 1 beside 16-bit items: ub0 = 32 only when max_user + 1 is formed without overflow, and then 16 + 32 + 16 = 64
        "int32_user_packed": (spread(U, 0, INT32_MAX), dense_to(I, 2 ** 16 - 1)),
    }
    # nRU + nRI = 2^25 and one more, the items dense: max_user + 1 + (I + 1)
    p["shard_edge_on"] = (dense_to(U, SHARD_MAX_RAW_IDS - (I + 1) - 1), dense(I))
    p["shard_edge_off"] = (dense_to(U, SHARD_MAX_RAW_IDS - (I + 1)), dense(I))
    for f, g in p.values():
        for a in (f, g):
            assert a.dtype == np.int64 and np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] <= INT32_MAX
    return p


def relabel(ids, f):
    """Dense 1-based ids -> raw ids.  Negative ids (a stray entry of a clustering map) pass through unchanged; an id above len(f) has no
    image -- a caller that wants an id above every raw id builds it from f[-1] itself."""
    ids = np.asarray(ids, dtype=np.int64)
    inside = ids >= 1
    assert np.all(ids[inside] <= len(f)) and not np.any(ids == 0)
    out = ids.copy()
    out[inside] = f[ids[inside] - 1]
    return out.astype(np.int32)


def unlabel(raw, f):
    """Raw ids -> dense 1-based ids; every id must be one of f's."""
    raw = np.asarray(raw, dtype=np.int64)
    at = np.searchsorted(f, raw)
    assert np.all(at < len(f)) and np.array_equal(f[np.minimum(at, len(f) - 1)], raw), "an id that the relabelling never produced"
    return (at + 1).astype(np.int32)


def relabel_triples(triples, f, g):
    user, item, score = triples
    return relabel(user, f), relabel(item, g), np.asarray(score, dtype=np.float32)


# which map every id column of a job's output goes back through
USER_KEYS = ("user", "user_id", "rec_user")
ITEM_KEYS = ("item", "other", "item_id", "rec_item", "a", "b")


def map_back(out, f, g):
    """A job's output (a dict of arrays and scalars) with every raw id column mapped back to dense ids; everything else untouched."""
    back = {}
    for k, v in out.items():
        if k in USER_KEYS:
            back[k] = unlabel(v, f)
        elif k in ITEM_KEYS:
            back[k] = unlabel(v, g)
        else:
            back[k] = v
    return back
