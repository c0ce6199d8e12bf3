"""The contract of fy_ratings_apply (include/filmyou.h, rules 1-6 and the counters) in plain Python: a dict keyed by (user, item) and
order bookkeeping, no product code.  The yardstick of tests/test_ratings_update_gpu.py."""
import numpy as np

COUNTERS = ("n_writes", "n_superseded", "n_replaced", "n_inserted", "n_deleted", "n_delete_missed", "n_source_dropped", "nnz_out")


def apply_writes(src_user, src_item, src_score, user, item, score, remove=None):
    """-> (user int32, item int32, score float32, counters dict).  The source triples and the batch are sequences of equal length;
    `remove` is None or one truth value per write."""
    src = list(zip((int(x) for x in src_user), (int(x) for x in src_item), (np.float32(x) for x in src_score)))
    n = len(user)
    assert n == len(item) == len(score) and (remove is None or len(remove) == n)
    # rule 1: replaying the batch row by row leaves the last write per key -- (position, score, is a delete)
    last = {}
    for p in range(n):
        last[(int(user[p]), int(item[p]))] = (p, np.float32(score[p]), bool(remove[p]) if remove is not None else False)
    # rule 2: every source entry whose key the batch names is dropped (all copies of a duplicate); rule 3: survivors in source order
    in_source = {(u, i) for u, i, _ in src}
    kept = [(u, i, s) for u, i, s in src if (u, i) not in last]
    # rule 3: ... followed by the last writes that are not deletes, by batch position; rule 4: the score as given, whatever its sign
    live = sorted((p, key, s) for key, (p, s, gone) in last.items() if not gone)
    rows = kept + [(key[0], key[1], s) for _, key, s in live]
    c = dict.fromkeys(COUNTERS, 0)
    c["n_writes"] = n
    c["n_superseded"] = n - len(last)
    for key, (_, _, gone) in last.items():
        c[("n_deleted" if gone else "n_replaced") if key in in_source else ("n_delete_missed" if gone else "n_inserted")] += 1
    c["n_source_dropped"] = len(src) - len(kept)
    c["nnz_out"] = len(rows)
    assert c["nnz_out"] == len(src) - c["n_source_dropped"] + c["n_replaced"] + c["n_inserted"]
    return (np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows], dtype=np.int32),
            np.array([r[2] for r in rows], dtype=np.float32), c)


def same_bits(a, b):
    """Two float32 arrays hold the same bit patterns (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
