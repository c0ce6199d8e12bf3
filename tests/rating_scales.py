"""Score patterns on both sides of the RM2 job's value gate, over (user, item) structures the suite already has.

The job takes the packed row walk (4-byte CSR entries, fixed-point sums, bit-reproducible) when every kept rating is exactly
representable in fp16, and the unpacked walk (8-byte entries, fp64 atomics) otherwise (fy_rm2_plan.hpp: use_pk).  Every other data set
of the suite holds integers or half stars.  Here the (user, item) pairs stay those of

    "small"   test_score_walk_gpu.dataset(False): 900 x 700, three 256-column chunks, lists of 1 ... 699
    "wide"    test_cooc_epilogue_gpu.wide_dataset(): 600 x 2 400, two epilogue trips
    "ml100k"  synth.generate("ml100k"): 943 x 1 682, whole stars

and only the scores change, each a function of (user, item) alone (mix(), SEED):

    "half"         the structure's own half stars                                                                  packed
    "tenths"       float32(k / 10), k = 1 ... 50: about 80 % are not fp16-exact                                    unpacked
    "continuous"   log-uniform in [0.05, 300], full 24-bit mantissas                                               unpacked
    "one_inexact"  the half stars with ONE rating set to float32(3.3), on an item of the last chunk                unpacked
    "dyadic"       a 2^-9 with integer 1 <= a < 4096, every user's ratings moved until they sum to a power of two  unpacked
    "pow2_0" / "pow2_13" / "pow2_14"   integers 1 ... 5 times 1, 2^13, 2^14: 40960 fits fp16, 65536 and 81920 do not  packed / packed / unpacked

"dyadic": about a quarter of the a need 12 significant bits (fp16 has 11), so the job is unpacked without a knob; x = r / s is exact
in fp32, a contribution x_vi x_vj is exact in fp64 and so is every sum of them (tests/test_rating_scales_cpu.py shows it with
integers): the fp64 accumulators hold exact sums whatever the order of the atomics and the matrix is a pure function of the data.
"pow2_*": the same problem at three magnitudes -- sums stay integers (quirk Q1's floor does nothing) and every operation of the
estimator scales exactly, so the oracle's rows are the same floats.

Test infrastructure only; tests/test_rating_scales_cpu.py proves the patterns are what tests/test_rating_scales_gpu.py needs."""
import functools

import numpy as np

import oracle

SEED = 1                    # a pattern whose oracle rows fall below |score| = 1 is re-seeded (test_rating_scales_cpu.py), never granted an absolute term
PATTERNS = ("tenths", "continuous", "one_inexact", "dyadic", "pow2_0", "pow2_13", "pow2_14")
STRUCTURES = ("small", "wide", "ml100k")
DYADIC_SHIFT = 9            # a dyadic rating is a 2^-9
INEXACT = np.float32(3.3)


@functools.lru_cache(maxsize=None)
def structure(name):
    """-> (user, item, the structure's own scores, numberOfItems)"""
    if name == "small":
        from test_score_walk_gpu import N_ITEMS, dataset
        return dataset(False) + (N_ITEMS,)
    if name == "wide":
        from test_cooc_epilogue_gpu import WIDE_ITEMS, wide_dataset
        return wide_dataset() + (WIDE_ITEMS,)
    assert name == "ml100k"
    from util import synth
    u, i, s, facts = synth().generate("ml100k")
    return u.numpy(), i.numpy(), s.numpy(), facts["n_items"]


def mix(user, item, stream=0):
    """32 well-mixed bits per (user, item): the finaliser of splitmix64 over a linear combination of the ids.  int64 in [0, 2^32)."""
    with np.errstate(over="ignore"):
        x = (np.asarray(user).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.asarray(item).astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F)
             + np.uint64(SEED * 1000 + stream) * np.uint64(0xD6E8FEB86659FD93))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(32)).astype(np.int64)


def not_fp16_exact(s):
    """The library's criterion (fy_prep.hip / k_discount_not_fp16) restated: a value that does not survive fp32 -> fp16 -> fp32; overflow to
    inf counts as inexact."""
    s = np.asarray(s, dtype=np.float32)
    with np.errstate(over="ignore"):
        return s.astype(np.float16).astype(np.float32) != s


def the_inexact_entry(name):
    """Index of the rating that "one_inexact" replaces (and that the update test writes): the lowest user of an item 37 columns before the
    last -- inside the last chunk under every chunk width the tests force."""
    user, item, _, n_items = structure(name)
    at = np.flatnonzero(item == n_items - 37)
    return int(at[np.argmin(user[at])])


@functools.lru_cache(maxsize=None)
def dyadic_units(name):
    """The integers a of "dyadic" (rating = a 2^-9), in the order of the structure's entries: 1 + hash mod 4095, then every user's a moved by
    equal steps (inside 1 ... 4095) until they sum to the power of two nearest to their sum -- one always lies in [n, 4095 n]."""
    user, item, _, _ = structure(name)
    a = 1 + mix(user, item, 4) % 4095
    order = np.argsort(user, kind="stable")
    bounds = np.flatnonzero(np.diff(user[order])) + 1
    for idx in np.split(order, bounds):
        v = a[idx]
        n, total = len(v), int(v.sum())
        powers = [p for p in (1 << k for k in range(0, 40)) if n <= p <= 4095 * n]
        assert powers
        want = min(powers, key=lambda p: abs(p - total))
        delta = want - total
        while delta:
            sign = 1 if delta > 0 else -1
            room = (4095 - v) if delta > 0 else (v - 1)
            free = np.flatnonzero(room > 0)
            q = abs(delta) // len(free)
            if q == 0:
                free, q = free[:abs(delta)], 1
            step = np.minimum(room[free], q)
            v[free] += sign * step
            delta -= sign * int(step.sum())
        a[idx] = v
    return a


@functools.lru_cache(maxsize=None)
def scores(pattern, name):
    user, item, own, _ = structure(name)
    if pattern == "half":
        return own
    if pattern == "tenths":
        return ((1 + mix(user, item, 1) % 50) / 10.0).astype(np.float32)
    if pattern == "continuous":
        t = mix(user, item, 2) / 4294967296.0
        return (0.05 * (300.0 / 0.05) ** t).astype(np.float32)
    if pattern == "one_inexact":
        s = own.copy()
        s[the_inexact_entry(name)] = INEXACT
        return s
    if pattern == "dyadic":
        return (dyadic_units(name).astype(np.float64) / (1 << DYADIC_SHIFT)).astype(np.float32)
    if pattern == "plus_2^-12":          # k + 2^-12, k = the half star rounded up: inexact; minus 2^-12 it is an integer
        return (np.ceil(own.astype(np.float64)) + 2.0 ** -12).astype(np.float32)
    assert pattern.startswith("pow2_")
    return ((1 + mix(user, item, 3) % 5) * float(1 << int(pattern[5:]))).astype(np.float32)


def triples(pattern, name):
    """"one_removed": the structure's own scores without the entry that "one_inexact" replaces"""
    user, item, own, _ = structure(name)
    if pattern == "one_removed":
        keep = np.arange(len(user)) != the_inexact_entry(name)
        return user[keep], item[keep], own[keep]
    return user, item, scores(pattern, name)


def n_items_of(name):
    return structure(name)[3]


@functools.lru_cache(maxsize=None)
def clustering(name, K):
    """(users, clusters): one cluster, or synth.hash_clustering"""
    from util import synth
    uu = np.unique(structure(name)[0])
    return uu, (np.zeros(len(uu), dtype=np.int32) if K == 1 else synth().hash_clustering(uu, K))


def oracle_of(trip, n_items, lam, K, clust):
    return oracle.rm2(*trip, lam=float(lam), number_of_items=n_items, number_of_recommendations=1 << 30, number_of_clusters=K,
                      map_user=clust[0], map_cluster=clust[1], n_threads=16)


@functools.lru_cache(maxsize=None)
def reference(pattern, name, lam="0.1", K=1):
    """The oracle's full ranking (an unbounded list), once per (pattern, structure, lambda, clusters); the half stars of "small" and
    "wide" in one cluster share the runs of the files they come from."""
    if pattern == "half" and K == 1 and name == "small":
        from test_score_walk_gpu import reference as small_reference
        return small_reference(False, lam)
    if pattern == "half" and K == 1 and name == "wide" and lam == "0.1":
        from test_cooc_rect_gpu import wide_reference
        return wide_reference()
    return oracle_of(triples(pattern, name), n_items_of(name), lam, K, clustering(name, K))


@functools.lru_cache(maxsize=None)
def smoothing_reference(pattern, name, method, param):
    """tests/rm2_smoothing_definition.py on one cluster: every candidate of every user"""
    from rm2_smoothing_definition import definition_full
    return definition_full(*triples(pattern, name), method, param, n_items_of(name))


# what tests/test_rating_scales_gpu.py compares at util.RTOL with no absolute term: (pattern, structure, lambda, clusters, list length)
ORACLE_CASES = (
    ("tenths", "small", "0.1", 1, 10), ("continuous", "small", "0.1", 1, 10), ("one_inexact", "small", "0.1", 1, 10),
    ("tenths", "small", "0.0", 1, 10), ("tenths", "wide", "0.1", 1, 10), ("pow2_13", "small", "0.1", 1, 10), ("pow2_14", "small", "0.1", 1, 10),
    ("dyadic", "small", "0.1", 1, 10), ("dyadic", "wide", "0.1", 1, 10), ("tenths", "small", "0.1", 1, 100),
    ("half", "small", "0.1", 1, 10), ("half", "wide", "0.1", 1, 10), ("tenths", "wide", "0.1", 6, 10), ("half", "wide", "0.1", 6, 10),
    ("tenths", "ml100k", "0.1", 20, 30), ("tenths", "ml100k", "0.1", 1, 20), ("one_removed", "small", "0.1", 1, 10),
    ("plus_2^-12", "small", "0.1", 1, 10),
)
DELTA_OUT, DELTA_IN = 0.3, 2.0 ** -12       # half stars minus 0.3 leave the packed walk; k + 2^-12 minus 2^-12 enters it
SMOOTHING_CASES = (("half", "small", "absoluteDiscounting", DELTA_OUT, 10), ("plus_2^-12", "small", "absoluteDiscounting", DELTA_IN, 10))
