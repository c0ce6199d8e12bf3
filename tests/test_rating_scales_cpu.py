"""The score patterns of tests/rating_scales.py are what tests/test_rating_scales_gpu.py needs them to be.  No GPU.

  * which side of the fp16 gate a pattern is on, by the kernel's own criterion restated in numpy (rating_scales.not_fp16_exact), with the
    expected share of inexact ratings; "one_inexact" has exactly one;
  * the side outputs are exact: every user sum and item sum is a sum of multiples of the smallest ulp among the fp32 scores, and the
    largest of them is below 2^53 of those units -- in integers, no float is trusted -- so an fp64 sum is the same number in every
    order and the GPU tests compare user_sum / total_sum / item sums for equality;
  * "dyadic": every user's ratings sum to a power of two, float32(r) / float32(s) in fp32 is the rational r / s, and every element of
    X^T X in the common unit is an integer below 2^53: the fp64 atomics of the unpacked walk add exact numbers to exact sums, so the
    byte identities the GPU file asserts between the variants of that walk are identities of the code, not of luck;
  * "pow2_*": the oracle's rows for x1, x2^13, x2^14 are the same floats;
  * the suite's tolerance is purely relative (util.RTOL, atol = 0): the oracle's top-N rows of every case the GPU file compares have
    |score| >= 1.  A pattern that fails here is re-seeded (rating_scales.SEED), it is never granted an absolute term.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import rating_scales as RS
from util import full_ranking

GATE = [(p, s) for s in ("small", "wide", "ml100k") for p in ("half",) + RS.PATTERNS + ("plus_2^-12",)]
# share of ratings that are not fp16-exact: (low, high)
SHARE = {"half": (0.0, 0.0), "tenths": (0.75, 0.85), "continuous": (0.99, 1.0), "dyadic": (0.2, 0.3), "pow2_0": (0.0, 0.0), "pow2_13": (0.0, 0.0),
         "pow2_14": (0.35, 0.45), "plus_2^-12": (1.0, 1.0)}


@pytest.mark.parametrize("pattern,name", GATE)
def test_side_of_the_fp16_gate(pattern, name):
    s = RS.scores(pattern, name)
    assert s.dtype == np.float32 and len(s) == len(RS.structure(name)[0]) and np.all(s > 0) and np.all(np.isfinite(s))
    bad = RS.not_fp16_exact(s)
    if pattern == "one_inexact":
        at = RS.the_inexact_entry(name)
        assert int(bad.sum()) == 1 and bad[at] and s[at] == RS.INEXACT
        own = RS.scores("half", name)
        assert np.array_equal(np.delete(s, at), np.delete(own, at)) and own[at] != RS.INEXACT
        user, item, _, n_items = RS.structure(name)
        assert item[at] - 1 >= 256 * ((n_items - 1) // 256)         # the last 256-column block: the last chunk under every chunk width
        return
    share = float(bad.mean())
    print(pattern, name, "share of ratings that are not fp16-exact: %.4f" % share)
    lo, hi = SHARE[pattern]
    assert lo <= share <= hi
    if pattern == "tenths":
        assert set(np.unique(s).tolist()) == {float(np.float32(k / 10)) for k in range(1, 51)}
    if pattern == "continuous":
        assert 0.05 <= s.min() < 0.06 and 250 < s.max() <= 300
        assert np.mean(s.view(np.uint32) & 1) > 0.4                 # the last mantissa bit is in use: full 24-bit mantissas
    if pattern.startswith("pow2_"):
        k = int(pattern[5:])
        assert set(np.unique(s).tolist()) == {float(m << k) for m in range(1, 6)}
        assert np.array_equal(bad, s >= 65536.0)                    # the gate is crossed by overflow, not by mantissa
        assert np.array_equal(s, RS.scores("pow2_0", name) * np.float32(1 << k))
    if pattern == "plus_2^-12":
        back = (s.astype(np.float64) - RS.DELTA_IN).astype(np.float32)
        assert np.array_equal(back, np.rint(back)) and not RS.not_fp16_exact(back).any()


def test_discounted_half_stars_leave_the_packed_walk():
    """r - 0.3 in fp64, rounded to fp32 as the library stores r': no half star stays fp16-exact"""
    r = RS.scores("half", "small")
    back = (r.astype(np.float64) - RS.DELTA_OUT).astype(np.float32)
    assert not RS.not_fp16_exact(r).any() and RS.not_fp16_exact(back).all()


def as_units(s):
    """fp32 scores as Python integers in units of the smallest ulp among them -> (list of ints, log2 of the unit)"""
    mant, exp = np.frexp(s.astype(np.float64))                       # s = mant 2^exp, 0.5 <= mant < 1: 24 bits of mant
    m = np.rint(mant * (1 << 24)).astype(np.int64)
    assert np.array_equal(m.astype(np.float64) / (1 << 24), mant)
    unit = int(exp.min()) - 24                                       # the ulp of the smallest binade in use
    return [int(a) << (int(e) - 24 - unit) for a, e in zip(m.tolist(), exp.tolist())], unit


@pytest.mark.parametrize("pattern,name", list(dict.fromkeys((c[0], c[1]) for c in RS.ORACLE_CASES + RS.SMOOTHING_CASES)))
def test_side_outputs_are_exact_in_fp64(pattern, name):
    user, item, s = RS.triples(pattern, name)
    units, unit = as_units(s)
    by_user, by_item = {}, {}
    for u, i, a in zip(user.tolist(), item.tolist(), units):
        by_user[u] = by_user.get(u, 0) + a
        by_item[i] = by_item.get(i, 0) + a
    largest = max(max(by_user.values()), max(by_item.values()))
    print(pattern, name, "unit 2^%d, largest sum %d bits" % (unit, largest.bit_length()))
    assert largest < 1 << 53
    # and the fp64 sums in numpy's order are those integers
    su = np.bincount(user, weights=s.astype(np.float64))
    assert all(int(su[u] * 2.0 ** -unit) == v for u, v in by_user.items())


@pytest.mark.parametrize("name", ["small", "wide"])
def test_dyadic_sums_are_exact(name):
    user, item, s = RS.triples("dyadic", name)
    a = RS.dyadic_units(name)
    assert a.min() >= 1 and a.max() <= 4095 and np.array_equal(s.astype(np.float64) * (1 << RS.DYADIC_SHIFT), a)
    uu, ux = np.unique(user, return_inverse=True)
    iu, ix = np.unique(item, return_inverse=True)
    total = np.bincount(ux, weights=a).astype(np.int64)              # (below 2^53: exact)
    assert np.all(total & (total - 1) == 0), "a user's ratings do not sum to a power of two"
    k = np.log2(total).astype(np.int64)
    assert np.array_equal(1 << k, total)
    # x = r / s in fp32, as the library divides, is the rational a / 2^k
    s_user = (total.astype(np.float64) / (1 << RS.DYADIC_SHIFT)).astype(np.float32)
    x32 = s / s_user[ux]
    assert x32.dtype == np.float32 and np.array_equal(x32.astype(np.float64) * total[ux], a)
    # X^T X in the common unit 2^(-2 kmax): integers, int64 (no wrap: users x the largest scaled square stays below 2^63)
    kmax = int(k.max())
    scaled = a << (kmax - k[ux])
    assert len(uu) * int(scaled.max()) ** 2 < 1 << 63
    X = sp.csr_matrix((scaled.astype(np.int64), (ux, ix)), shape=(len(uu), len(iu)))
    G = (X.T @ X).tocoo()
    assert G.dtype == np.int64
    bits = int(G.data.max()).bit_length()
    print(name, "k = %d ... %d, largest element of X^T X: %d bits" % (int(k.min()), kmax, bits))
    assert int(G.data.max()) < 1 << 53 and G.data.min() > 0
    # a contribution x_vi x_vj is exact in fp64 (24 + 24 bits) and in the common unit
    assert int(scaled.max()) ** 2 < 1 << 53


def same_rows(a, b):
    return all(np.array_equal(a[k].view(np.int32) if k == "rec_score" else a[k], b[k].view(np.int32) if k == "rec_score" else b[k])
               for k in ("rec_user", "rec_item", "rec_score", "rec_cluster"))


def test_pow2_rows_are_the_same_floats():
    r0, r13, r14 = (RS.reference("pow2_%d" % k, "small") for k in (0, 13, 14))
    assert len(r0["rec_user"]) > 0 and same_rows(r0, r13) and same_rows(r0, r14)
    assert r0["log_terms"] == r13["log_terms"] == r14["log_terms"]
    assert np.array_equal(r13["user_sum"], r0["user_sum"] * 8192.0) and r14["total_sum"] == r0["total_sum"] * 16384.0


def least_of_the_lists(ref, top_n):
    least = np.inf
    for items, sc, _ in full_ranking(ref).values():
        top = sc[:top_n]
        fin = np.isfinite(top)
        if fin.any():
            least = min(least, float(np.abs(top[fin]).min()))
    return least


@pytest.mark.parametrize("pattern,name,lam,K,top_n", RS.ORACLE_CASES)
def test_list_scores_are_no_smaller_than_one(pattern, name, lam, K, top_n):
    ref = RS.reference(pattern, name, lam, K)
    least = least_of_the_lists(ref, top_n)
    print(pattern, name, lam, K, top_n, "smallest |score| of the lists: %.3f" % least)
    assert least >= 1.0
    if lam == "0.0":
        assert np.isneginf(ref["rec_score"]).any()


@pytest.mark.parametrize("pattern,name,method,param,top_n", RS.SMOOTHING_CASES)
def test_smoothing_list_scores_are_no_smaller_than_one(pattern, name, method, param, top_n):
    least = least_of_the_lists(RS.smoothing_reference(pattern, name, method, param), top_n)
    print(pattern, name, method, param, "smallest |score| of the lists: %.3f" % least)
    assert least >= 1.0
