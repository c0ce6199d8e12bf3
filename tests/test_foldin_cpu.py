"""Fold-in of given profiles (fy_foldin_*), the parts that need no GPU: the numpy statement of tests/foldin_ref.py against the
reference's own vectors and against the factorisation oracle, the composition rules on a hand-made case, and the refusals the library
makes before it touches a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import foldin_ref as FR
import oracle
from util import pkg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factorization_test_data.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name,ppc", [("nmf", False), ("ppc", True)])
def test_statement_reproduces_the_reference_vectors(golden, name, ppc):
    """One iteration from H_init with W_init held is H_one: the fold-in IS the reference's H update (test_nmf_gpu.py's tolerance)."""
    d = golden[name]
    ref = FR.assign(np.array(d["W_init"]), FR.profiles_of_columns(d["A"]), iterations=1, first_iteration=1, ppc=ppc, f=12, h0=np.array(d["H_init"]))
    worst = np.max(np.abs(ref["H"] - np.array(d["H_one"])))
    print("%s: worst difference to H_one %.2e" % (name, worst))
    np.testing.assert_allclose(ref["H"], np.array(d["H_one"]), rtol=0, atol=1e-9)
    assert (ref["status"] == FR.OK).all() and min(ref["margin"]) > 1e-9


def test_statement_reproduces_the_ppc_toy(golden):
    d = golden["ppc"]
    ref = FR.assign(np.array(d["w0p"]), FR.profiles_of_columns(d["Ap"]), iterations=1, ppc=True, f=12, h0=np.array(d["h0p"]))
    np.testing.assert_allclose(ref["H"], np.array(d["h1p"]), rtol=0, atol=1e-7)


@pytest.mark.parametrize("ppc,f", [(False, 0), (True, 0), (True, -1)])
def test_statement_equals_the_factorisation_oracle(ppc, f):
    rng = np.random.default_rng(3 + f)
    n_users, n_items, k = 40, 30, 6
    A = (rng.random((n_items, n_users)) < 0.3) * rng.integers(1, 6, (n_items, n_users))
    A[rng.integers(0, n_items, n_users), np.arange(n_users)] = 3
    A[np.arange(n_items), rng.integers(0, n_users, n_items)] = 4
    i, u = np.nonzero(A)
    H0, W0 = rng.random((n_users, k)) + 0.01, rng.random((n_items, k)) + 0.01
    Ho, _ = oracle.nmf((u + 1).astype(np.int32), (i + 1).astype(np.int32), A[i, u].astype(np.float32), H0, W0, iterations=1, ppc=ppc,
                       normalization_frequency=f)
    ref = FR.assign(W0, FR.profiles_of_columns(A), iterations=1, ppc=ppc, f=f, h0=H0)
    np.testing.assert_allclose(ref["H"], Ho, rtol=1e-12, atol=0)      # two fp64 evaluations of one formula: sums of <= 30 terms
    if ppc and f == -1:
        np.testing.assert_allclose(np.abs(ref["H"]).sum(1), 1.0, rtol=1e-12)


def test_composition_rules_and_counters():
    n_items = 10
    #            dup(last wins)  delete      <= 0 / NaN          outside          unsorted
    items = [7, 3, 7,         5, 5,       2, 9, 4,            0, -3, 11,       8, 1]
    score = [1.0, 2.0, 4.5,   3.0, 9.0,   0.0, -1.0, np.nan,  5.0, 5.0, 5.0,   2.5, 3.5]
    remove = [0, 0, 0,        0, 1,       0, 0, 0,            0, 0, 0,         0, 0]
    got_items, got_scores, c = FR.compose(n_items, items, score, remove)
    assert got_items.tolist() == [1, 3, 7, 8] and got_scores.tolist() == [3.5, 2.0, 4.5, 2.5]
    assert c == dict(out_of_range=3, superseded=2, removed=1, nonpositive=3)
    # a delete that is superseded by a later write does not delete
    got_items, _, c = FR.compose(n_items, [5, 5], [1.0, 2.0], [1, 0])
    assert got_items.tolist() == [5] and c["removed"] == 0 and c["superseded"] == 1
    # everything gone: the profile is empty
    ref = FR.assign(np.ones((n_items, 2)), [(1, [0, 3], [1.0, 0.0])], iterations=1)
    assert ref["status"].tolist() == [FR.EMPTY] and ref["clusters"].tolist() == [-1] and ref["parents"].tolist() == [-1]


def test_statuses_and_masks_of_the_statement():
    W = np.array([[1.0, 5.0, 2.0], [1.0, 4.0, 3.0]])
    prof = [(1, [1, 2], [1.0, 1.0])]
    assert FR.assign(W, prof, iterations=0)["clusters"].tolist() == [0]                       # uniform start: the first index
    assert FR.assign(W, prof, iterations=0, counts=[0, 0, 4])["clusters"].tolist() == [2]     # ... the first ALLOWED index
    free = FR.assign(W, prof, iterations=2, ppc=False)
    assert free["clusters"].tolist() == [1]
    masked = FR.assign(W, prof, iterations=2, ppc=False, counts=[3, 0, 1])
    assert masked["clusters"].tolist() == [2] and np.array_equal(masked["H"], free["H"])      # the mask touches only the argmax
    none = FR.assign(W, prof, iterations=2, counts=[0, 0, 0])
    assert none["status"].tolist() == [FR.NO_CLUSTER] and none["clusters"].tolist() == [-1]
    level = dict(items=[[1], [2], [5]], W=[np.ones((1, 2)), np.array([[1.0, 2.0, 3.0]]), np.ones((1, 1))], stride=2, counts=None)
    two = FR.assign(W, prof, iterations=2, ppc=False, level=level)
    assert two["parents"].tolist() == [1] and two["clusters"].tolist() == [1 * 2 + 2] and two["counters"]["collisions"] == 1
    level["items"][1] = [9]
    gone = FR.assign(W, prof, iterations=2, ppc=False, level=level)
    assert gone["status"].tolist() == [FR.EMPTY_IN_PARENT] and gone["parents"].tolist() == [1] and gone["clusters"].tolist() == [-1]


def test_argument_validation_without_a_device():
    P = pkg()
    P.build()
    lib = P._native.load()
    W = np.ones((4, 2))
    cnt = np.ones(2, np.int32)

    def create(params, w, location, count, n_count, out, ctx=None):
        return lib.fy_foldin_create(ctx, C.byref(params) if params is not None else None, w, location, count, n_count, out)

    good = P._native.FoldInParams(4, 2, 1, -1)
    assert create(good, W.ctypes.data, 0, None, 0, None) == -1 and b"out" in lib.fy_last_error()
    out = C.c_void_p(1)
    assert create(None, W.ctypes.data, 0, None, 0, C.byref(out)) == -1 and out.value is None and b"params" in lib.fy_last_error()
    for bad in (P._native.FoldInParams(0, 2, 1, -1), P._native.FoldInParams(4, 0, 1, -1)):
        out = C.c_void_p(1)
        assert create(bad, W.ctypes.data, 0, None, 0, C.byref(out)) == -1 and out.value is None
    out = C.c_void_p(1)
    assert create(P._native.FoldInParams(4, 257, 1, -1), W.ctypes.data, 0, None, 0, C.byref(out)) == -10 and out.value is None      # FY_ERR_UNSUPPORTED
    assert b"256" in lib.fy_last_error()
    out = C.c_void_p(1)
    assert create(good, None, 0, None, 0, C.byref(out)) == -1 and b"W is NULL" in lib.fy_last_error()
    assert create(good, W.ctypes.data, 2, None, 0, C.byref(out)) == -1 and b"location" in lib.fy_last_error()
    assert create(good, W.ctypes.data, 0, None, 2, C.byref(out)) == -1 and b"count" in lib.fy_last_error()
    assert create(good, W.ctypes.data, 0, cnt.ctypes.data, -1, C.byref(out)) == -1 and b"count" in lib.fy_last_error()
    assert create(good, W.ctypes.data, 0, cnt.ctypes.data, 2, C.byref(out)) == -1 and b"context is NULL" in lib.fy_last_error()
    assert out.value is None
    # the calls on a model: NULL model, NULL out
    assert lib.fy_foldin_add_level(None, 2, cnt.ctypes.data, cnt.ctypes.data, cnt.ctypes.data, W.ctypes.data, 1, None, 0) == -1
    assert b"NULL" in lib.fy_last_error()
    q = P._native.ItemCFProfiles(0, None, None, None, None, None, 0)
    out = C.c_void_p(1)
    assert lib.fy_foldin_assign(None, C.byref(q), 1, 1, None, 0, 1, C.byref(out)) == -1 and out.value is None
    assert lib.fy_foldin_assign(None, C.byref(q), 1, 1, None, 0, 1, None) == -1 and b"out" in lib.fy_last_error()
    assert lib.fy_foldin_result_n(None) == 0 and lib.fy_foldin_result_sub_size(None) == 0
    assert lib.fy_foldin_result_assignment(None, None, None, None, None) == -1
    assert lib.fy_foldin_result_factors(None, None) == -1 and lib.fy_foldin_result_sub_factors(None, None, None) == -1
    assert lib.fy_foldin_result_stats(None, None) == -1
    lib.fy_foldin_result_free(None)
    lib.fy_foldin_destroy(None)


def test_header_library_and_bindings_agree():
    P = pkg()
    S = P._native.FoldInStats
    assert C.sizeof(P._native.FoldInParams) == 16 and C.sizeof(S) == 19 * 8
    assert [getattr(S, f).offset for f, _ in S._fields_] == list(range(0, 19 * 8, 8))
    assert (P.FY_FOLDIN_OK, P.FY_FOLDIN_EMPTY, P.FY_FOLDIN_NO_CLUSTER, P.FY_FOLDIN_EMPTY_IN_PARENT) == (FR.OK, FR.EMPTY, FR.NO_CLUSTER, FR.EMPTY_IN_PARENT)
    assert hasattr(P, "FoldIn") and hasattr(P, "FoldInAssignment")
    assert P._native.load().fy_abi_version() == 5      # additions only
