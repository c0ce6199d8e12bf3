"""numpy restatements for the cluster-refinement tests (test_refine_cpu.py, test_refine_gpu.py): the seed generator of
include/filmyou.h, SubClusterMappingJob's semantics, and the refinement composed from what the project could already
express -- host extraction, oracle.nmf per parent cluster, oracle.cluster_assign with the offsets."""
import numpy as np

import oracle



def mix(x):
    """splitmix64's step on uint64 arrays (wrapping)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def initial_matrix(seed, cluster, which, n_rows, k):
    """Matrix `which` (0 = H, 1 = W) of parent `cluster`: the formula in include/filmyou.h, values in (0, 1]."""
    row = np.arange(n_rows, dtype=np.uint64)[:, None]
    col = np.arange(k, dtype=np.uint64)[None, :]
    a = mix((row << np.uint64(32)) | col)
    b = mix(((np.uint64(cluster) << np.uint64(32)) | np.uint64(which)) ^ a)
    z = mix(np.uint64(seed) ^ b)
    return ((z >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53


def mappings(user, item, score, map_user, map_cluster, K):
    """SubClusterMappingJob in numpy.  Returns a dict:
    users[c] / items[c]: ascending raw ids (new id = position + 1); kept: mask over the COO; row_user / row_item: global row
    (cluster-major) of every kept rating."""
    user, item, score = np.asarray(user), np.asarray(item), np.asarray(score)
    cl = {}
    for a, b in zip(np.asarray(map_user).tolist(), np.asarray(map_cluster).tolist()):
        cl[a] = b                                   # a later entry replaces the earlier
    users = [np.array(sorted(x for x, c in cl.items() if c == k), dtype=np.int64) for k in range(K)]
    keep = score > 0
    get_cluster = np.array([cl.get(x, 0) for x in user.tolist()], dtype=np.int64)      # Trove's no-entry value
    items = [np.unique(item[keep & (get_cluster == k)]).astype(np.int64) for k in range(K)]
    member = np.array([x in cl for x in user.tolist()], dtype=bool)
    kept = keep & member
    ustart = np.r_[0, np.cumsum([len(x) for x in users])]
    istart = np.r_[0, np.cumsum([len(x) for x in items])]
    ru, ri = np.zeros(kept.sum(), np.int64), np.zeros(kept.sum(), np.int64)
    ku, ki, kc = user[kept], item[kept], get_cluster[kept]
    for k in range(K):
        sel = kc == k
        ru[sel] = ustart[k] + np.searchsorted(users[k], ku[sel])
        ri[sel] = istart[k] + np.searchsorted(items[k], ki[sel])
    return {"users": users, "items": items, "kept": kept, "row_user": ru, "row_item": ri, "ustart": ustart, "istart": istart,
            "cluster_of": cl}


def csr(rows, cols, vals, n_rows):
    order = np.lexsort((cols, rows))
    ptr = np.r_[0, np.cumsum(np.bincount(rows, minlength=n_rows))]
    return ptr.astype(np.int32), cols[order].astype(np.int32), vals[order].astype(np.float32)


def extract(user, item, score, m, c):
    """Parent c's submatrix as 1-based COO in the new ids."""
    kept = m["kept"]
    ku, ki, ks = np.asarray(user)[kept], np.asarray(item)[kept], np.asarray(score)[kept]
    sel = (m["row_user"] >= m["ustart"][c]) & (m["row_user"] < m["ustart"][c + 1])
    nu = np.searchsorted(m["users"][c], ku[sel]) + 1
    ni = np.searchsorted(m["items"][c], ki[sel]) + 1
    return nu.astype(np.int32), ni.astype(np.int32), ks[sel].astype(np.float32)


def sub_clusters(m, users_per_sub_cluster):
    return [-(-len(x) // users_per_sub_cluster) for x in m["users"]]


def composed_refinement(user, item, score, map_user, map_cluster, K, users_per_sub_cluster, number_of_users, iterations, ppc,
                        normalization_frequency, H0, W0):
    """Host extraction, oracle.nmf per parent, oracle.cluster_assign with the offsets.  H0 / W0: lists per parent.
    Returns (users, clusters, counts, [(H_c, W_c)], near_tie mask): near_tie marks the users whose two largest entries of
    their oracle row differ by no more than 1e-8 relative."""
    m = mappings(user, item, score, map_user, map_cluster, K)
    kc = sub_clusters(m, users_per_sub_cluster)
    stride = -(-number_of_users // K)
    n_counts = max([K * stride] + [c * stride + kc[c] for c in range(K) if kc[c] > 0])
    counts = np.zeros(n_counts, np.int64)
    us, cs, factors, ties = [], [], [], []
    for c in range(K):
        if len(m["users"][c]) == 0:
            factors.append((np.zeros((0, 0)), np.zeros((len(m["items"][c]), 0))))
            continue
        u, i, s = extract(user, item, score, m, c)
        H, W = oracle.nmf(u, i, s, H0[c], W0[c], iterations=iterations, ppc=ppc, normalization_frequency=normalization_frequency)
        factors.append((H, W))
        _, cl = oracle.cluster_assign(H, first_user=1, cluster_offset=c * stride)
        us.append(m["users"][c])
        cs.append(cl)
        np.add.at(counts, cl, 1)
        top = np.sort(H, axis=1)[:, ::-1]
        ties.append((top[:, 0] - top[:, 1] <= 1e-8 * np.abs(top[:, 0])) if H.shape[1] > 1 else np.zeros(len(H), bool))
    return (np.concatenate(us).astype(np.int32), np.concatenate(cs).astype(np.int32), counts.astype(np.int32), factors,
            np.concatenate(ties), m)


def ml100k_case():
    """The refined-clustering case of both test files: the ML-100K-shaped synthetic with dense ids, 5 hashed parents."""
    from util import synth
    S = synth()
    u, i, s, _ = S.generate("ml100k")
    u, i, s = u.numpy(), i.numpy(), s.numpy()
    uu, u = np.unique(u, return_inverse=True)
    ii, i = np.unique(i, return_inverse=True)
    u, i = (u + 1).astype(np.int32), (i + 1).astype(np.int32)
    users = np.arange(1, len(uu) + 1, dtype=np.int32)
    return {"coo": (u, i, s), "n_users": len(uu), "n_items": len(ii), "K": 5, "users_per_sub_cluster": 50,
            "map_user": users, "map_cluster": S.hash_clustering(users, 5), "iterations": 10, "normalization_frequency": 12,
            "seeds": (11, 2024)}


def seeded_initial(m, kc, seed):
    H0 = [initial_matrix(seed, c, 0, len(m["users"][c]), kc[c]) for c in range(len(kc))]
    W0 = [initial_matrix(seed, c, 1, len(m["items"][c]), kc[c]) for c in range(len(kc))]
    return H0, W0


DRIVER_PPC_SEED = 4


def driver_initial(n_users, n_items, K, seed):
    """RMRecommenderDriver.run's draw of the top-level PPC run's initial matrices, restated: H first, then W, both in (0, 1]."""
    rng = np.random.default_rng(seed)
    H = 1.0 - rng.random((n_users, K))
    W = 1.0 - rng.random((n_items, K))
    return H, W


def driver_ppc_stage(case, seed, iterations=10, normalization_frequency=12):
    """The driver's first stage from the oracles: PPC with the driver's defaults, then the argmax.  Returns (users, clusters,
    counts, near_tie mask, H0, W0); near_tie as in composed_refinement."""
    u, i, s = case["coo"]
    H0, W0 = driver_initial(case["n_users"], case["n_items"], case["K"], seed)
    H, _ = oracle.nmf(u, i, s, H0, W0, iterations=iterations, ppc=True, normalization_frequency=normalization_frequency)
    users, clusters, counts = oracle.cluster_assign(H, first_user=1, n_clusters=case["K"])
    top = np.sort(H, axis=1)[:, ::-1]
    ties = top[:, 0] - top[:, 1] <= 1e-8 * np.abs(top[:, 0])
    return users, clusters, counts, ties, H0, W0
