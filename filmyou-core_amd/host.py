"""Host side of the drop-in: the reference's job interface re-stated over the C ABI.

Mirrors (same names, argument meaning, error behaviour):
  * Hadoop ``Configuration`` with the keys of M/rmrecommender/RMRecommenderDriver.java:49-120
  * ``RM2Job.run`` (M/rm/RM2Job.java:76-100): returns 0-equivalent (a result object) or raises
    ``RuntimeError("<job> failed!: ...")`` like RM2Job.java:144-147
  * ``RowSimilarityJob.run`` with the option names passed at M/baselinerecommender/BaselineRecommenderJob.java:241-253
The reference's Cassandra / HDFS readers and writers stay on the Java side (north_star: unchanged); this layer takes
the rating triples they produce and returns the rows they consume.
"""
import ctypes as C
import os

import numpy as np

from . import _native

SIMILARITY_COSINE = "SIMILARITY_COSINE"
SIMILARITY_COOCCURRENCE = "SIMILARITY_COOCCURRENCE"
SIMILARITY_TANIMOTO_COEFFICIENT = "SIMILARITY_TANIMOTO_COEFFICIENT"
SIMILARITY_LOGLIKELIHOOD = "SIMILARITY_LOGLIKELIHOOD"
SIMILARITY_CITY_BLOCK = "SIMILARITY_CITY_BLOCK"
SIMILARITY_EUCLIDEAN_DISTANCE = "SIMILARITY_EUCLIDEAN_DISTANCE"
SIMILARITY_PEARSON_CORRELATION = "SIMILARITY_PEARSON_CORRELATION"
# name -> FY_SIMILARITY_* of include/filmyou.h (Mahout 0.8's VectorSimilarityMeasures, in its order)
_SIMILARITY = {SIMILARITY_COSINE: 0, SIMILARITY_COOCCURRENCE: 1, SIMILARITY_TANIMOTO_COEFFICIENT: 2, SIMILARITY_LOGLIKELIHOOD: 3,
               SIMILARITY_CITY_BLOCK: 4, SIMILARITY_EUCLIDEAN_DISTANCE: 5, SIMILARITY_PEARSON_CORRELATION: 6}
# Mahout's measure classes, as --similarityClassname also takes them; the reference's own default is String.valueOf(X.class),
# i.e. the name with "class " in front (BaselineRecommenderJob.java:163)
_MEASURES_PACKAGE = "org.apache.mahout.math.hadoop.similarity.cooccurrence.measures."
_SIMILARITY_CLASS = {"CosineSimilarity": 0, "CooccurrenceCountSimilarity": 1, "TanimotoCoefficientSimilarity": 2,
                     "LoglikelihoodSimilarity": 3, "CityBlockSimilarity": 4, "EuclideanDistanceSimilarity": 5,
                     "PearsonCorrelationSimilarity": 6}


def similarity_id(similarityClassname):
    """FY_SIMILARITY_* for a --similarityClassname value: a SIMILARITY_* name or a fully qualified Mahout measure class,
    with or without a leading "class ".  Anything else is a ValueError."""
    name = similarityClassname
    if name in _SIMILARITY:
        return _SIMILARITY[name]
    if isinstance(name, str):
        if name.startswith("class "):
            name = name[len("class "):]
        if name.startswith(_MEASURES_PACKAGE) and name[len(_MEASURES_PACKAGE):] in _SIMILARITY_CLASS:
            return _SIMILARITY_CLASS[name[len(_MEASURES_PACKAGE):]]
    raise ValueError("similarityClassname must be one of %s or a measure class of %s*" % (", ".join(_SIMILARITY), _MEASURES_PACKAGE))


class FilmYouError(RuntimeError):
    """A non-zero fy_status from the native library."""

    def __init__(self, code, message):
        super().__init__("fy_status %d: %s" % (code, message))
        self.code = code
        self.message = message


def _check(rc):
    if rc != 0:
        raise FilmYouError(rc, _native.load().fy_last_error().decode(errors="replace"))


class Configuration(dict):
    """The slice of org.apache.hadoop.conf.Configuration the jobs read: string values, typed getters with defaults."""

    # option names of RMRecommenderDriver (M/rmrecommender/RMRecommenderDriver.java:49-120) and their defaults
    DEFAULTS = {"lambda": "0.1", "numberOfRecommendations": "1000", "clusterSplit": "400", "splitSize": "100",
                "filterUsers": "0", "directory": "recommendation", "clustering": "clustering",
                "clusteringCount": "clusteringCount"}

    def set(self, key, value):
        self[key] = str(value)

    def setInt(self, key, value):
        self[key] = str(int(value))

    def setFloat(self, key, value):
        # Configuration.setFloat stores Float.toString(value): 0.5f -> "0.5" (quirk Q3)
        self[key] = str(np.float32(value))

    def setBoolean(self, key, value):
        self[key] = "true" if value else "false"

    def get(self, key, default=None):
        if key in self:
            return dict.get(self, key)
        return self.DEFAULTS.get(key, default)

    def getInt(self, key, default):
        v = self.get(key)
        return int(v) if v is not None else default

    def getDouble(self, key, default):
        v = self.get(key)
        return float(v) if v is not None else default

    def getBoolean(self, key, default):
        v = self.get(key)
        return (str(v).lower() == "true") if v is not None else default


class Context:
    """One GPU, one HIP stream (fy_context)."""

    def __init__(self, device=0):
        self._lib = _native.load()
        h = C.c_void_p()
        _check(self._lib.fy_context_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self._tuning_env = self._fy_env()

    @staticmethod
    def _fy_env():
        return tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("FY_")))

    def sync_tuning(self):
        """The library reads its FY_* knobs (test / measurement hooks) from the environment once, at fy_context_create.  This
        host mirror re-reads them (fy_context_reload_tuning) when the process environment has changed since -- the parity tests
        switch paths per test on one context; a production job never gets here with a changed environment."""
        env = self._fy_env()
        if env != self._tuning_env:
            _check(self._lib.fy_context_reload_tuning(self._h))
            self._tuning_env = env

    def synchronize(self):
        _check(self._lib.fy_context_synchronize(self._h))

    def inject_alloc_failure(self, nth):
        """Fault injection (tests): the nth HBM request from now fails with FY_ERR_OUT_OF_MEMORY; 0 disarms."""
        _check(self._lib.fy_context_inject_alloc_failure(self._h, int(nth)))

    @property
    def stream(self):
        return self._lib.fy_context_stream(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fy_context_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _is_torch_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


class Ratings:
    """Rating triples in HBM.  Accepts numpy arrays (copied over PCIe) or torch tensors already on the context's GPU."""

    def __init__(self, ctx, user, item, score):
        self._lib = _native.load()
        self.ctx = ctx
        if _is_torch_tensor(user):
            import torch
            assert user.is_cuda and item.is_cuda and score.is_cuda, "device tensors expected"
            assert user.dtype == torch.int32 and item.dtype == torch.int32 and score.dtype == torch.float32
            user, item, score = user.contiguous(), item.contiguous(), score.contiguous()
            torch.cuda.current_stream(user.device).synchronize()   # producer stream != the context's stream
            n, ptrs, loc = user.numel(), (user.data_ptr(), item.data_ptr(), score.data_ptr()), 1
        else:
            user = np.ascontiguousarray(user, dtype=np.int32)
            item = np.ascontiguousarray(item, dtype=np.int32)
            score = np.ascontiguousarray(score, dtype=np.float32)
            n, ptrs, loc = len(user), (user.ctypes.data, item.ctypes.data, score.ctypes.data), 0
        assert n == len(item) == len(score)
        self._keep = (user, item, score)
        h = C.c_void_p()
        _check(self._lib.fy_ratings_create(ctx._h, n, ptrs[0], ptrs[1], ptrs[2], loc, C.byref(h)))
        self._h = h
        self._keep = None
        self.nnz = n

    @classmethod
    def _adopt(cls, ctx, handle, nnz):
        r = cls.__new__(cls)
        r._lib, r.ctx, r._keep, r._h, r.nnz = _native.load(), ctx, None, handle, nnz
        return r

    def shifted(self, shift):
        """fy_ratings_shifted: a new Ratings whose scores are float32(score + shift) -- the reference's ratingShift
        (BaselineToItemPrefsMapper.java:60).  Nothing the jobs kept on this object is carried over."""
        h = C.c_void_p()
        _check(self._lib.fy_ratings_shifted(self.ctx._h, self._h, float(shift), C.byref(h)))
        return Ratings._adopt(self.ctx, h, self.nnz)

    def updated(self, user, item, score, remove=None):
        """fy_ratings_apply: a new Ratings from this one and a batch of writes (user, item, score[, remove]) taken in order, with
        the ratings table's semantics -- the last write per (user, item) counts, a write replaces the stored row, a non-zero
        `remove` entry deletes it (include/filmyou.h states the rules).  Numpy arrays or torch tensors on the context's GPU
        (remove: uint8 / bool).  This object is only read: what the jobs kept on it stays valid; the new object starts with
        none.  The counters are in ``.update_stats`` of the result."""
        self.ctx.sync_tuning()
        if _is_torch_tensor(user):
            import torch
            assert user.is_cuda and item.is_cuda and score.is_cuda and (remove is None or remove.is_cuda), "device tensors expected"
            assert user.dtype == torch.int32 and item.dtype == torch.int32 and score.dtype == torch.float32
            user, item, score = user.contiguous(), item.contiguous(), score.contiguous()
            if remove is not None:
                remove = (remove != 0).to(torch.uint8).contiguous()
            torch.cuda.current_stream(user.device).synchronize()   # producer stream != the context's stream
            n, loc = user.numel(), 1
            ptrs = (user.data_ptr(), item.data_ptr(), score.data_ptr(), remove.data_ptr() if remove is not None else None)
            n_remove = n if remove is None else remove.numel()
        else:
            user = np.ascontiguousarray(user, dtype=np.int32)
            item = np.ascontiguousarray(item, dtype=np.int32)
            score = np.ascontiguousarray(score, dtype=np.float32)
            if remove is not None:
                remove = np.ascontiguousarray(np.asarray(remove) != 0, dtype=np.uint8)
            n, loc = len(user), 0
            ptrs = (user.ctypes.data, item.ctypes.data, score.ctypes.data, remove.ctypes.data if remove is not None else None)
            n_remove = n if remove is None else len(remove)
        assert n == len(item) == len(score) == n_remove
        h, st = C.c_void_p(), _native.RatingsUpdateStats()
        _check(self._lib.fy_ratings_apply(self.ctx._h, self._h, n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], loc, C.byref(h), C.byref(st)))
        r = Ratings._adopt(self.ctx, h, st.nnz_out)
        r.update_stats = st.as_dict()
        return r

    def holdout(self, fraction, seed=0):
        """fy_ratings_holdout: ``(train, test)``, two new Ratings.  A rating goes to ``test`` by a hash of its (user, item) and
        ``seed`` alone (include/filmyou.h states it), so its side does not change when other ratings are written; both sides
        keep this object's order and the scores' bits.  This object is only read."""
        tr, te = C.c_void_p(), C.c_void_p()
        _check(self._lib.fy_ratings_holdout(self.ctx._h, self._h, float(fraction), int(seed) & (2 ** 64 - 1), C.byref(tr), C.byref(te)))
        return (Ratings._adopt(self.ctx, tr, int(self._lib.fy_ratings_nnz(tr))), Ratings._adopt(self.ctx, te, int(self._lib.fy_ratings_nnz(te))))

    def to_host(self):
        """fy_ratings_copy_out: (user, item, score) numpy arrays of the COO as it lives in HBM, in its order."""
        n = int(self._lib.fy_ratings_nnz(self._h))
        user, item, score = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float32)
        _check(self._lib.fy_ratings_copy_out(self._h, user.ctypes.data, item.ctypes.data, score.ctypes.data))
        return user, item, score

    def drop_cache(self):
        """fy_ratings_drop_cache: releases what earlier jobs kept on this object (CSR / CSC, statistics, row-kernel tables)."""
        if getattr(self, "_h", None) and self.ctx._h:
            self._lib.fy_ratings_drop_cache(self._h)

    def close(self):
        if getattr(self, "_h", None):
            if self.ctx._h:
                self._lib.fy_ratings_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _np(ptr, n, dtype):
    if not ptr or n == 0:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype).copy()


class _Result:
    def __init__(self, handle, ctx=None):
        self._lib = _native.load()
        self._h = handle
        self._ctx = ctx   # rows are downloaded through the context's stream: keep it alive

    def _stats(self):
        st = _native.Stats()
        _check(self._lib.fy_result_stats(self._h, C.byref(st)))
        return st.as_dict()

    def close(self):
        if getattr(self, "_h", None):
            if self._ctx is None or self._ctx._h:   # a result must not outlive its context's stream
                self._lib.fy_result_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Recommendations(_Result):
    """Rows of the `recommendations` table / output SequenceFile: (user, item, relevance float32, cluster),
    grouped by user, best first -- plus the job's side outputs rm2/userSum and rm2/itemColl."""

    def __init__(self, handle, ctx=None):
        super().__init__(handle, ctx)
        L = self._lib
        self.stats = self._stats()
        self.size = L.fy_result_size(handle)
        self._rows = None
        self._sums = None
        # fy_rm2_score_users only: what the request touched (None on the result of a full job)
        rq = _native.RM2RequestStats()
        self.request_stats = rq.as_dict() if L.fy_result_request_stats(handle, C.byref(rq)) == 0 else None
        # fy_rm2_score_profiles only: fy_rm2_profile_stats (None on any other result)
        ps = _native.RM2ProfileStats()
        self.profile_stats = ps.as_dict() if L.fy_result_rm2_profile_stats(handle, C.byref(ps)) == 0 else None

    def rows(self):
        if self._rows is None:
            L, h, n = self._lib, self._h, self.size
            self._rows = {"user": _np(L.fy_result_key0(h), n, np.int32), "item": _np(L.fy_result_key1(h), n, np.int32),
                          "score": _np(L.fy_result_value(h), n, np.float32),
                          "cluster": _np(L.fy_result_aux(h), n, np.int32)}
        return self._rows

    def sums(self):
        if self._sums is None:
            L, h = self._lib, self._h
            nu, ni = L.fy_result_n_users(h), L.fy_result_n_items(h)
            self._sums = {"user_id": _np(L.fy_result_user_id(h), nu, np.int32),
                          "user_sum": _np(L.fy_result_user_sum(h), nu, np.float64),
                          "item_id": _np(L.fy_result_item_id(h), ni, np.int32),
                          "item_coll": _np(L.fy_result_item_coll(h), ni, np.float64),
                          "total_sum": L.fy_result_total_sum(h)}
        return self._sums


class ItemSimilarities(_Result):
    """Rows of the similarity matrix: (item, other item, similarity), grouped by item, best first."""

    def __init__(self, handle, ctx=None, request=False):
        super().__init__(handle, ctx)
        self.stats = self._stats()
        self.size = self._lib.fy_result_size(handle)
        self._rows = None
        # request=True (a result of fy_itemsim_rows): what the request touched; None on the result of a full build
        self.request_stats = None
        if request:
            rq = _native.ItemSimRequestStats()
            _check(self._lib.fy_result_itemsim_request_stats(handle, C.byref(rq)))
            self.request_stats = rq.as_dict()

    def rows(self):
        if self._rows is None:
            L, h, n = self._lib, self._h, self.size
            self._rows = {"item": _np(L.fy_result_key0(h), n, np.int32), "other": _np(L.fy_result_key1(h), n, np.int32),
                          "sim": _np(L.fy_result_value(h), n, np.float32)}
        return self._rows

    def pairs(self):
        """fy_itemsim_pairs: the matrix as de-duplicated item pairs {"a": min id, "b": max id, "sim"}, sorted by (a, b) -- what the
        reference's outputPathForSimilarityMatrix job writes (BaselineRecommenderJob.java:259-278).  Rows of a world == 1 build."""
        res = C.c_void_p()
        _check(self._lib.fy_itemsim_pairs(self._ctx._h, self._h, C.byref(res)))
        L = self._lib
        try:
            n = L.fy_result_size(res)
            return {"a": _np(L.fy_result_key0(res), n, np.int32), "b": _np(L.fy_result_key1(res), n, np.int32),
                    "sim": _np(L.fy_result_value(res), n, np.float32)}
        finally:
            L.fy_result_free(res)


def read_id_file(path):
    """fy_idfile_read: the ids of a usersFile / itemsFile (one per line; lines that are not an int32 are skipped)."""
    lib = _native.load()
    n, ids = C.c_int64(), C.c_void_p()
    _check(lib.fy_idfile_read(os.fsencode(path), C.byref(n), C.byref(ids)))
    try:
        return _np(ids.value, n.value, np.int32)
    finally:
        lib.fy_buffer_free(ids)


def write_similarity_pairs(path, pairs):
    """fy_simpairs_write_text: `a<TAB>b<TAB>sim` lines from ItemSimilarities.pairs()."""
    a, b = _i32(pairs["a"]), _i32(pairs["b"])
    sim = np.ascontiguousarray(pairs["sim"], dtype=np.float32)
    assert len(a) == len(b) == len(sim)
    _check(_native.load().fy_simpairs_write_text(os.fsencode(path), len(a), a.ctypes.data, b.ctypes.data, sim.ctypes.data))


def _id_list(ids):
    """usersFile= / itemsFile=: a path or an integer array; None = option off."""
    if ids is None:
        return None
    if isinstance(ids, (str, bytes, os.PathLike)):
        return read_id_file(ids)
    return _i32(ids)


def _i32(a):
    return np.ascontiguousarray(a if a is not None else [], dtype=np.int32)


def _pair_ids(a):
    """ids of asked pairs: every pair is answered, so an id outside int32 cannot be passed over -- it is refused"""
    a = np.asarray(a).reshape(-1)
    if a.dtype != np.int32:
        a = np.asarray(a, dtype=np.int64) if len(a) else np.zeros(0, dtype=np.int64)
        if ((a < -2 ** 31) | (a >= 2 ** 31)).any():
            raise ValueError("an id of a pair is outside int32")
    return np.ascontiguousarray(a, dtype=np.int32)


def _profile_items(a):
    """raw item ids of profile entries: an id outside int32 is outside the data -- it becomes -1, which has no column and is counted"""
    a = np.asarray(a).reshape(-1)
    if a.dtype != np.int32:
        a = np.asarray(a, dtype=np.int64) if len(a) else np.zeros(0, dtype=np.int64)
        a = np.where((a < -2 ** 31) | (a >= 2 ** 31), -1, a)
    return np.ascontiguousarray(a, dtype=np.int32)


def _itemcf_profiles(profiles, base, shift):
    """``profiles`` of ``PreparedItemSimilarity.recommend_profiles`` -> (fy_itemcf_profiles, what must stay alive while it is used)"""
    if base not in ("whole", "resident"):
        raise ValueError("base must be 'whole' or 'resident'")
    if isinstance(profiles, tuple) and len(profiles) in (4, 5) and isinstance(profiles[0], np.ndarray):      # the CSR arrays
        labels, start, item, score = profiles[:4]
        remove = profiles[4] if len(profiles) == 5 else None
        start = np.ascontiguousarray(start, dtype=np.int64).reshape(-1)
    else:
        labels, lens, items, scores, removes = [], [], [], [], []
        any_remove = False
        for prof in profiles:
            if len(prof) not in (3, 4):
                raise ValueError("a profile is (label, items, scores) or (label, items, scores, remove)")
            it = np.asarray(prof[1]).reshape(-1)
            sc = np.asarray(prof[2], dtype=np.float32).reshape(-1)
            rm = np.zeros(len(it), dtype=np.uint8) if len(prof) == 3 or prof[3] is None else (np.asarray(prof[3]).reshape(-1) != 0).astype(np.uint8)
            if not len(it) == len(sc) == len(rm):
                raise ValueError("items, scores and remove of a profile differ in length")
            any_remove = any_remove or (len(prof) == 4 and prof[3] is not None)
            labels.append(prof[0]); lens.append(len(it)); items.append(it); scores.append(sc); removes.append(rm)
        start = np.zeros(len(labels) + 1, dtype=np.int64)
        np.cumsum(lens, out=start[1:])
        item = np.concatenate(items) if items else np.zeros(0, dtype=np.int64)
        score = np.concatenate(scores) if scores else np.zeros(0, dtype=np.float32)
        remove = np.concatenate(removes) if any_remove else None
    labels = _pair_ids(labels)
    item = _profile_items(item)
    score = np.ascontiguousarray(score, dtype=np.float32).reshape(-1)
    if shift != 0.0:
        score = score + np.float32(shift)      # float32(score + shift): Ratings.shifted's arithmetic
    if remove is not None:
        remove = np.ascontiguousarray(np.asarray(remove).reshape(-1) != 0, dtype=np.uint8)
    n = len(labels)
    if len(start) != n + 1 and not (n == 0 and len(start) == 0):
        raise ValueError("start must hold one offset more than there are profiles")
    if len(item) != len(score) or (remove is not None and len(remove) != len(item)) or (n and int(start[-1]) > len(item)):
        raise ValueError("item, score and remove must hold start[-1] entries each")
    ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
    q = _native.ItemCFProfiles(n, ptr(labels), start.ctypes.data if len(start) else None, ptr(item), ptr(score), ptr(remove),
                               _native.FY_PROFILE_ON_RESIDENT if base == "resident" else _native.FY_PROFILE_WHOLE)
    return q, (labels, start, item, score, remove)


def _rm2_profiles(profiles, base, clusters, rank, world):
    """``profiles`` of ``PreparedRM2.score_profiles`` (the two forms ``recommend_profiles`` takes) -> (fy_rm2_profiles, what must stay
    alive while it is used).  ``clusters``: one cluster for all profiles or one per profile; required with base="whole"."""
    q, keep = _itemcf_profiles(profiles, base, 0.0)
    n = q.n_profiles
    cl = None
    if clusters is not None:
        cl = np.asarray(clusters).reshape(-1)
        if cl.size == 1 and n != 1:
            cl = np.repeat(cl, n)
        cl = _pair_ids(cl)
        if len(cl) != n:
            raise ValueError("clusters must hold one cluster, or one per profile")
    elif base == "whole" and n > 0:
        raise ValueError("base='whole' needs clusters=: the cluster every profile is scored in")
    r = _native.RM2Profiles(n, q.user, q.start, q.item, q.score, q.remove, cl.ctypes.data if cl is not None and len(cl) else None, q.base,
                            int(rank), int(world))
    return r, (keep, cl)


def _itemcf_pairs(pairs):
    """``(users, items)`` raw-id arrays (numpy, or int32 torch tensors on the context's GPU) -> (fy_itemcf_pairs, what must stay alive
    while it is used)"""
    users, items = pairs
    if _is_torch_tensor(users):
        import torch
        assert users.is_cuda and items.is_cuda, "device tensors expected"
        assert users.dtype == torch.int32 and items.dtype == torch.int32
        users, items = users.contiguous(), items.contiguous()
        torch.cuda.current_stream(users.device).synchronize()   # producer stream != the context's stream
        n, ptrs, loc = users.numel(), (users.data_ptr(), items.data_ptr()), 1
        assert n == items.numel()
    else:
        users, items = _pair_ids(users), _pair_ids(items)
        n, ptrs, loc = len(users), (users.ctypes.data, items.ctypes.data), 0
        assert n == len(items)
    return _native.ItemCFPairs(n, ptrs[0] if n else None, ptrs[1] if n else None, loc), (users, items)


class RM2Job:
    """Relevance Model 2 job (M/rm/RM2Job.java:54-272) on one MI355X (or one rank of several).

    ``conf`` carries the reference's keys: lambda, numberOfItems, numberOfClusters, numberOfRecommendations,
    filterUsers (clusterSplit / splitSize are accepted and ignored: they only partition the reference's reduce groups
    and never change a score -- M/common/AbstractByClusterAndCountMapper.java:86-102).

    Smoothing of the user language model (include/filmyou.h, FY_RM2_SMOOTHING_*): ``smoothing`` = ``jm`` (the default: the
    reference's Jelinek-Mercer, parameter ``lambda``), ``dirichlet`` (parameter ``mu``) or ``absoluteDiscounting`` (parameter
    ``delta``), matched without regard to case.  ``mu`` / ``delta`` have no default: the chosen method's parameter must be set.

    Estimator: ``relevanceModel`` = ``rm2`` (the default, the reference's) or ``rm1`` (FY_RM2_ESTIMATOR_RM1: the paper's RM1 over the
    same neighbourhoods and the same user model, one fp64 pass; include/filmyou.h), matched without regard to case; anything else
    is a ValueError.  ``PreparedRM2.score_users`` and ``run(usersFile=)`` follow the job's estimator."""

    JOB_NAME = "RM2"
    # smoothing name (lower case) -> (flag bit of fy_rm2_params::flags, the Configuration key of the method's parameter)
    SMOOTHING = {"jm": (0, "lambda"), "dirichlet": (2, "mu"), "absolutediscounting": (4, "delta")}
    # relevanceModel (lower case) -> flag bit: rm2 (the default, the reference's estimator) or rm1 (FY_RM2_ESTIMATOR_RM1)
    RELEVANCE_MODEL = {"rm2": 0, "rm1": 8}

    def __init__(self, conf, ctx=None):
        self.conf = conf
        self.ctx = ctx

    def _params(self, rank, world, workspace_bytes):
        conf = self.conf
        n_clusters = conf.getInt("numberOfClusters", -1)
        n_items = conf.getInt("numberOfItems", -1)
        if n_clusters is None or n_clusters <= 0 or n_items is None or n_items <= 0:
            # AbstractJob.parseArguments rejects a missing required option (TestRMRecommenderJob.java:39-74)
            raise ValueError("numberOfClusters and numberOfItems are required")
        name = str(conf.get("smoothing", "jm"))
        if name.lower() not in self.SMOOTHING:
            raise ValueError("smoothing must be jm, dirichlet or absoluteDiscounting (got %r)" % name)
        flag, key = self.SMOOTHING[name.lower()]
        if conf.get(key) is None:
            raise ValueError("smoothing=%s needs %s" % (name, key))
        lam = float(conf.get(key))    # (jm) Double.valueOf(conf.get("lambda")), AbstractRM2Reducer.java:108
        model = str(conf.get("relevanceModel", "rm2"))
        if model.lower() not in self.RELEVANCE_MODEL:
            raise ValueError("relevanceModel must be rm2 or rm1 (got %r)" % model)
        flag |= self.RELEVANCE_MODEL[model.lower()]
        return _native.RM2Params(lam, n_items, conf.getInt("numberOfRecommendations", 1000),
                                 conf.getInt("filterUsers", 0), n_clusters, int(rank), int(world), flag,
                                 int(workspace_bytes))

    def prepare(self, ratings, clustering=None, clustering_count=None, rank=0, world=1, workspace_bytes=0, cache=True):
        """Stage 1 (jobs RM2-1 / RM2-2 up to the exchange).  Returns a PreparedRM2 holding this rank's partial item
        statistics in HBM; see RM2Job.run for the arguments."""
        lib = _native.load()
        p = self._params(rank, world, workspace_bytes)
        if not cache:
            p.flags |= 1            # FY_RM2_NO_CACHE
        ctx = self.ctx or Context(0)
        self.ctx = ctx
        own_ratings = not isinstance(ratings, Ratings)
        r = Ratings(ctx, *ratings) if own_ratings else ratings
        try:
            mu, mc = (_i32(clustering[0]), _i32(clustering[1])) if clustering is not None else (_i32(None), _i32(None))
            if len(mu) != len(mc):
                raise ValueError("clustering users / clusters differ in length")
            cc = None
            if clustering_count is not None:
                cc = np.zeros(p.number_of_clusters, dtype=np.int32)
                k = min(len(clustering_count), p.number_of_clusters)
                cc[:k] = np.asarray(clustering_count, dtype=np.int32)[:k]
            job = C.c_void_p()
            try:
                ctx.sync_tuning()
                _check(lib.fy_rm2_prepare(ctx._h, C.byref(p), r._h, len(mu), mu.ctypes.data, mc.ctypes.data,
                                          cc.ctypes.data if cc is not None else None, C.byref(job)))
            except FilmYouError as e:
                raise RuntimeError("%s failed!: %s" % (self.JOB_NAME, e.message)) from e
            return PreparedRM2(job, ctx, world)
        finally:
            if own_ratings:
                r.close()

    def run(self, ratings, clustering=None, clustering_count=None, rank=0, world=1, exchange=None,
            workspace_bytes=0, collectives=None, cache=True, usersFile=None):
        """ratings: a ``Ratings`` or a (user, item, score) triple of arrays.
        usersFile: a path of one user id per line (read_id_file) or an integer array: lists for these users alone, with the work
          sized by the request (PreparedRM2.score_users); None = the whole job.  Not with collectives= (ValueError).
        clustering: (users, clusters) arrays = the reference's `clustering` file; None routes everyone to cluster 0.
        clustering_count: array of numberOfClusters sizes = the `clusteringCount` file (validated when given).
        world > 1 needs one of
          collectives: an object with ``all_gather(send_ptr, recv_ptr, nbytes, stream_ptr)`` and
            ``reduce_scatter_f32(send_ptr, recv_ptr, count, stream_ptr)`` on device pointers (parallel.TorchCollectives =
            RCCL through torch.distributed): the statistics are all-gathered inside the library and clusters that span
            all ranks are scored cooperatively (every rank builds 1/world of the co-rating matrix);
          exchange(device_ptr, length) -> device_ptr of world*length doubles: only the all-gather of the per-item
            statistics (parallel.StatsExchange); every rank then builds the whole matrix of the clusters it holds users of.
        cache: a ``Ratings`` object keeps what the job built from the ratings and the clustering alone (CSR / CSC, per-item
          statistics, the row kernel's tables); a later job over the same object and the same clustering starts from it
          (stats["prepared_from_cache"]).  cache=False = FY_RM2_NO_CACHE: build everything, keep nothing (the cold job).
        Raises RuntimeError("RM2 failed!: ...") on any failure, like RM2Job.java:144-147."""
        if usersFile is not None and collectives is not None:
            raise ValueError("usersFile cannot be combined with collectives: the cooperative path serves no requests")
        if world > 1 and exchange is None and collectives is None:
            raise ValueError("world > 1 needs collectives (or at least an exchange for the item statistics)")
        users = _id_list(usersFile)
        prepared = self.prepare(ratings, clustering, clustering_count, rank, world, workspace_bytes, cache=cache)
        try:
            if collectives is not None:
                prepared.set_collectives(collectives)
            elif world > 1:
                ptr, n = prepared.partial_stats()
                prepared.set_global_stats(exchange(ptr, n))
            if users is not None:
                return prepared.score_users(users)
            return prepared.score()
        finally:
            prepared.close()


    def run_from_files(self, rank=0, world=1, **kw):
        """RM2Job.run on the reference's own file layout (M/rm/RM2Job.java:76-100, useCassandraInput/Output = false):
        ratings         <mapred.input.dir>                     SequenceFile<IntPairWritable(user,item), FloatWritable>
        clustering      <directory>/<clustering>               SequenceFile<IntWritable, IntWritable>
        clusteringCount <directory>/<clusteringCount>          SequenceFile<IntWritable, IntWritable>
        and writes      <directory>/rm2/userSum/part-r-00000   SequenceFile<IntWritable, DoubleWritable>
                        <directory>/rm2/itemColl/part-r-00000  MapFile<IntWritable, DoubleWritable> (data + index)
                        <mapred.output.dir>/part-r-00000       SequenceFile<IntPairWritable(user,item), FloatWritable>
        <directory>/rm2 is wiped first, like HadoopUtils.removeData (RM2Job.java:84).  Returns 0 (the Tool contract); a
        failure raises RuntimeError("RM2 failed!: ...").  Files: filmyou-core_amd/seqfile.py (layout parity unpinned)."""
        import shutil

        from . import seqfile
        conf = self.conf
        inp, outp = conf.get("mapred.input.dir"), conf.get("mapred.output.dir")
        base = conf.get("directory", "recommendation")
        if not inp or not outp:
            raise ValueError("mapred.input.dir and mapred.output.dir must be set (HadoopUtils.getInputPath / getOutputPath)")
        try:
            user, item, score = seqfile.read_intpair_float(inp)
            cu, cc = seqfile.read_int_int(os.path.join(base, conf.get("clustering", "clustering")))
            ck, cv = seqfile.read_int_int(os.path.join(base, conf.get("clusteringCount", "clusteringCount")))
        except seqfile.SeqFileError as e:
            raise RuntimeError("%s failed!: %s" % (self.JOB_NAME, e)) from e
        K = conf.getInt("numberOfClusters", -1)
        count = np.zeros(max(K, 1), dtype=np.int32)
        ok = (ck >= 0) & (ck < len(count))
        count[ck[ok]] = cv[ok]
        rm2 = os.path.join(base, "rm2")
        suffix = "part-r-%05d" % rank
        # Rank 0 alone wipes <directory>/rm2 (RM2Job.java:84), BEFORE its first collective: every other rank writes only after the
        # job, i.e. after a collective rank 0 has joined.  (The wipe comes before the output check, as in the reference: RM2Job.run
        # removes <directory>/rm2 at :84 and only the submission of job RM2-3 runs checkOutputSpecs -- a refused job has already lost
        # the previous run's statistics there too.)
        # mapred.output.dir is never deleted (the reference does not: Hadoop's FileOutputFormat.checkOutputSpecs refuses an existing
        # directory and the job fails).  One rank: an existing directory fails the job.  Several ranks share the directory, so it may
        # exist -- but it must not hold ANY part-r-* file, whoever wrote it (a rerun into the directory of a job with a larger world would
        # leave that job's other part files beside the new ones, and a reader of the directory would get stale rows without any
        # error).  No rank writes before it has passed a collective inside the job, which every rank joins only after this check: all
        # ranks see the same directory and fail together instead of hanging in a collective.
        if rank == 0:
            shutil.rmtree(rm2, ignore_errors=True)
        if world == 1:
            stale = [outp] if os.path.exists(outp) else []
        else:
            stale = sorted(f for f in (os.listdir(outp) if os.path.isdir(outp) else []) if f.startswith("part-r-"))
            if os.path.exists(outp) and not os.path.isdir(outp):
                stale = [outp]
        if stale:
            raise RuntimeError("%s failed!: output directory %s already exists%s" % (self.JOB_NAME, outp, "" if world == 1 else " and holds " + ", ".join(stale[:4])))
        if conf.get("usersFile") is not None and "usersFile" not in kw:
            kw["usersFile"] = conf.get("usersFile")
        rec = self.run((user, item, score), clustering=(cu, cc), clustering_count=count, rank=rank, world=world, **kw)
        try:
            rows = rec.rows()
            if rank == 0:       # rm2/userSum and rm2/itemColl are the GLOBAL statistics (jobs RM2-1 / RM2-2): one copy
                sums = rec.sums()
                seqfile.write_int_double(os.path.join(rm2, "userSum", "part-r-00000"), sums["user_id"], sums["user_sum"])
                seqfile.write_mapfile_int_double(os.path.join(rm2, "itemColl", "part-r-00000"), sums["item_id"], sums["item_coll"])
            seqfile.write_intpair_float(os.path.join(outp, suffix), rows["user"], rows["item"], rows["score"])
        finally:
            rec.close()
        return 0


class PreparedRM2:
    """A job between its two stages (fy_rm2_job): the CSR/CSC and this rank's partial statistics are in HBM."""

    def __init__(self, handle, ctx, world):
        self._lib = _native.load()
        self._h = handle
        self._ctx = ctx
        self.world = world

    def partial_stats(self):
        """(device pointer, length in doubles) of the exchange buffer: per-item partial rating sums in ascending raw
        item id order + this rank's partial of the floor-sum counter (x100) (+ user sums and a flag: stats_layout)."""
        buf, n = C.c_void_p(), C.c_int64()
        _check(self._lib.fy_rm2_partial_stats(self._h, C.byref(buf), C.byref(n)))
        return buf.value, n.value

    def stats_layout(self):
        """(n_item_slots, n_user_slots) of the exchange buffer: [n_item_slots item sums][floor-sum][n_user_slots user sums][flag if any user
        slots].  Replicated prep: one slot per rated item (ascending raw id), no user slots.  Sharded prep (several ranks, whole clusters per
        rank, a rank preps its own clusters' ratings alone): slots by RAW id, user sums and a failure flag behind the floor-sum."""
        ni, nu = C.c_int64(), C.c_int64()
        _check(self._lib.fy_rm2_stats_layout(self._h, C.byref(ni), C.byref(nu)))
        return ni.value, nu.value

    def set_global_stats(self, gathered_device_ptr):
        _check(self._lib.fy_rm2_set_global_stats(self._h, gathered_device_ptr, self.world))

    def set_collectives(self, comm):
        """Installs the process group's collectives (fy_rm2_set_collectives).  `comm.all_gather(send, recv, nbytes,
        stream)` / `comm.reduce_scatter_f32(send, recv, count, stream)` get raw device pointers and the hipStream_t the
        operation has to be ordered on; an exception inside them fails the job (FY_ERR_COLLECTIVE)."""
        self._comm_error = None
        if hasattr(comm, "native_struct"):       # compiled transport (parallel.RcclCollectives): C callbacks, no Python in the path
            self._coll = comm.native_struct
            self._keep_comm = comm
            _check(self._lib.fy_rm2_set_collectives(self._h, C.byref(self._coll)))
            return

        def guard(fn):
            def call(_user, send, recv, n, stream):
                try:
                    fn(send, recv, n, stream)
                    return 0
                except BaseException as e:      # must not unwind through the C frames
                    self._comm_error = e
                    return 1
            return call

        self._callbacks = (_native.ALL_GATHER_FN(guard(comm.all_gather)), _native.REDUCE_SCATTER_FN(guard(comm.reduce_scatter_f32)))
        self._coll = _native.Collectives(None, self._callbacks[0], self._callbacks[1])
        _check(self._lib.fy_rm2_set_collectives(self._h, C.byref(self._coll)))

    def score(self):
        res = C.c_void_p()
        try:
            try:
                self._ctx.sync_tuning()
                _check(self._lib.fy_rm2_score(self._h, C.byref(res)))
            except FilmYouError as e:
                if getattr(self, "_comm_error", None) is not None:
                    raise RuntimeError("%s failed!: collective: %r" % (RM2Job.JOB_NAME, self._comm_error)) from self._comm_error
                raise
        except FilmYouError as e:
            raise RuntimeError("%s failed!: %s" % (RM2Job.JOB_NAME, e.message)) from e
        return Recommendations(res, self._ctx)

    def score_users(self, ids):
        """fy_rm2_score_users: the rows score() would emit for the listed raw user ids (any order, duplicates and unknown ids
        passed over), with the work sized by the request.  Any number of calls, before or after score(); the job stays valid.
        Returns a ``Recommendations`` with ``request_stats`` beside ``stats``."""
        ids = np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int32)
        rq = _native.RM2Request(len(ids), ids.ctypes.data if len(ids) else None)
        res = C.c_void_p()
        try:
            self._ctx.sync_tuning()
            _check(self._lib.fy_rm2_score_users(self._h, C.byref(rq), C.byref(res)))
        except FilmYouError as e:
            raise RuntimeError("%s failed!: %s" % (RM2Job.JOB_NAME, e.message)) from e
        return Recommendations(res, self._ctx)

    def score_profiles(self, profiles, base="whole", clusters=None, rank=0, world=1):
        """fy_rm2_score_profiles: RM2 lists for item sets handed in -- an anonymous or new visitor's whole profile scored as one
        more member of a cluster (base="whole", ``clusters`` = one cluster or one per profile), or a resident user's row with
        pending writes applied (base="resident": the label is the user id, the cluster is that user's).  Only the SET of items
        matters; a score that is not > 0 removes the item, like a delete.  ``profiles``: a sequence of (label, items, scores) or
        (label, items, scores, remove) with the writes in order, or the CSR arrays (labels, start, item, score[, remove]).  The job
        stays as prepared and valid.  (rank, world) cut the profile list.  Returns a ``Recommendations`` with ``profile_stats``."""
        if profiles is None:
            raise ValueError("score_profiles() needs the profiles to score")
        q, keep = _rm2_profiles(profiles, base, clusters, rank, world)
        res = C.c_void_p()
        try:
            self._ctx.sync_tuning()
            _check(self._lib.fy_rm2_score_profiles(self._h, C.byref(q), C.byref(res)))
        except FilmYouError as e:
            raise RuntimeError("%s failed!: %s" % (RM2Job.JOB_NAME, e.message)) from e
        del keep
        return Recommendations(res, self._ctx)

    def close(self):
        if getattr(self, "_h", None):
            if self._ctx._h:
                self._lib.fy_rm2_job_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ItemRecommendations(_Result):
    """Rows of the item-based recommender's output table: (user, item, score), grouped by user, best first."""

    def __init__(self, handle, ctx=None, request=False):
        super().__init__(handle, ctx)
        self.stats = self._stats()
        self.size = self._lib.fy_result_size(handle)
        self._rows = None
        # request=True (a result of fy_itemcf_recommend_prepared): what the request touched; None on any other result
        self.request_stats = None
        # request="profiles" (a result of fy_itemcf_recommend_profiles): fy_itemcf_profile_stats; None on any other result
        self.profile_stats = None
        if request == "profiles":
            ps = _native.ItemCFProfileStats()
            _check(self._lib.fy_result_itemcf_profile_stats(handle, C.byref(ps)))
            self.profile_stats = ps.as_dict()
        elif request:
            rq = _native.ItemCFRequestStats()
            _check(self._lib.fy_result_itemcf_request_stats(handle, C.byref(rq)))
            self.request_stats = rq.as_dict()

    def rows(self):
        if self._rows is None:
            L, h, n = self._lib, self._h, self.size
            self._rows = {"user": _np(L.fy_result_key0(h), n, np.int32), "item": _np(L.fy_result_key1(h), n, np.int32),
                          "score": _np(L.fy_result_value(h), n, np.float32)}
        return self._rows

    @classmethod
    def from_rows(cls, ctx, user, item, score):
        """fy_result_create_lists: a list result from rows made elsewhere (the reference's own output read by
        seqfile.read_intpair_float, say), so that ``Evaluator.evaluate`` can take them.  Rows as given: grouped by user, best
        first; a user with two separate runs of rows is refused.  Numpy arrays or torch tensors on the context's GPU."""
        lib = _native.load()
        if _is_torch_tensor(user):
            import torch
            assert user.is_cuda and item.is_cuda and score.is_cuda, "device tensors expected"
            assert user.dtype == torch.int32 and item.dtype == torch.int32 and score.dtype == torch.float32
            user, item, score = user.contiguous(), item.contiguous(), score.contiguous()
            torch.cuda.current_stream(user.device).synchronize()   # producer stream != the context's stream
            n, ptrs, loc = user.numel(), (user.data_ptr(), item.data_ptr(), score.data_ptr()), 1
        else:
            user, item = _i32(user), _i32(item)
            score = np.ascontiguousarray(score, dtype=np.float32)
            n, ptrs, loc = len(user), (user.ctypes.data, item.ctypes.data, score.ctypes.data), 0
        assert n == len(item) == len(score)
        res = C.c_void_p()
        _check(lib.fy_result_create_lists(ctx._h, n, ptrs[0], ptrs[1], ptrs[2], loc, C.byref(res)))
        return cls(res, ctx)


class Evaluation:
    """What ``Evaluator.evaluate`` returns: the counters and, per cutoff, the SUMS over the evaluated lists (fy_eval_sums), as
    attributes and numpy arrays in cutoff order.  ``per_user`` (None unless asked for): {"user": ids in list order, "hits",
    "recall", "ap", "rr", "ndcg": lists x cutoffs float64, NaN for a list that was not evaluated}."""

    COUNTERS = ("lists", "users_evaluated", "lists_without_relevant", "relevant_users", "relevant_entries")
    SUMS = ("recall", "ap", "rr", "ndcg")

    def __init__(self, cutoffs, counters, hits, users_hit, sums, distinct_items=None, ms=0.0, per_user=None):
        self.cutoffs = tuple(int(c) for c in cutoffs)
        for k in self.COUNTERS:
            setattr(self, k, int(counters[k]))
        self.hits = np.asarray(hits, dtype=np.int64)
        self.users_hit = np.asarray(users_hit, dtype=np.int64)
        for k in self.SUMS:
            setattr(self, k, np.asarray(sums[k], dtype=np.float64))
        self.distinct_items = distinct_items
        self.ms = float(ms)
        self.per_user = per_user

    def means(self, count_missing=False):
        """{"precision", "recall", "map", "mrr", "ndcg", "hit_rate": arrays in cutoff order}: the sums over ``users_evaluated``;
        count_missing=True divides by ``relevant_users`` instead, so users with relevant test items and no list count as zeros.
        NaN where that count is 0."""
        d = float(self.relevant_users if count_missing else self.users_evaluated)
        d = d if d > 0 else float("nan")
        n = np.asarray(self.cutoffs, dtype=np.float64)
        return {"precision": self.hits / (n * d), "recall": self.recall / d, "map": self.ap / d, "mrr": self.rr / d,
                "ndcg": self.ndcg / d, "hit_rate": self.users_hit / d}

    @classmethod
    def merge(cls, parts):
        """The evaluation of a multi-rank job from its ranks' evaluations (each rank evaluates its own lists with an evaluator
        prepared from the same test ratings): counters and sums are added in the order given (rank order).  ``distinct_items`` is
        None (the union of the ranks' item sets is not formed) and ``per_user`` is dropped."""
        parts = list(parts)
        if not parts:
            raise ValueError("nothing to merge")
        first = parts[0]
        for p in parts[1:]:
            if p.cutoffs != first.cutoffs or p.relevant_users != first.relevant_users or p.relevant_entries != first.relevant_entries:
                raise ValueError("the evaluations come from different evaluators")
        counters = {k: sum(getattr(p, k) for p in parts) for k in ("lists", "users_evaluated", "lists_without_relevant")}
        counters["relevant_users"], counters["relevant_entries"] = first.relevant_users, first.relevant_entries
        sums = {}
        for k in cls.SUMS:
            acc = np.zeros(len(first.cutoffs), dtype=np.float64)
            for p in parts:
                acc = acc + getattr(p, k)
            sums[k] = acc
        return cls(first.cutoffs, counters, sum(p.hits for p in parts), sum(p.users_hit for p in parts), sums, None,
                   sum(p.ms for p in parts))


FY_ESTIMATE_OK, FY_ESTIMATE_UNKNOWN_USER, FY_ESTIMATE_UNKNOWN_ITEM, FY_ESTIMATE_OWN_PREFERENCE = 0, 1, 2, 3
FY_ESTIMATE_TOO_FEW, FY_ESTIMATE_ZERO_NUMERATOR, FY_ESTIMATE_NOT_A_NUMBER = 4, 5, 6


class EstimateErrors:
    """Rating-error SUMS of estimates against true scores (fy_eval_errors): ``pairs``, ``estimated`` (the OK rows with a finite
    truth score: what the sums run over), ``truth_not_finite``, ``by_status`` (rows per FY_ESTIMATE_* code), ``sum_abs``,
    ``sum_sq``, ``sum_err`` and ``ms``; the means are properties (NaN when nothing was estimated)."""

    def __init__(self, pairs, estimated, truth_not_finite, by_status, sum_abs, sum_sq, sum_err, ms=0.0):
        self.pairs, self.estimated, self.truth_not_finite = int(pairs), int(estimated), int(truth_not_finite)
        self.by_status = [int(x) for x in by_status]
        self.sum_abs, self.sum_sq, self.sum_err, self.ms = float(sum_abs), float(sum_sq), float(sum_err), float(ms)

    def _mean(self, x):
        return x / self.estimated if self.estimated > 0 else float("nan")

    @property
    def mae(self):
        return self._mean(self.sum_abs)

    @property
    def rmse(self):
        return float(np.sqrt(self._mean(self.sum_sq)))

    @property
    def bias(self):
        return self._mean(self.sum_err)

    @property
    def coverage(self):
        return self.estimated / self.pairs if self.pairs > 0 else float("nan")

    @classmethod
    def merge(cls, parts):
        """The errors of a multi-rank estimate from its ranks' errors: counters and sums are added in the order given (rank order)."""
        parts = list(parts)
        if not parts:
            raise ValueError("nothing to merge")
        sums = [0.0, 0.0, 0.0]
        for p in parts:
            sums = [sums[0] + p.sum_abs, sums[1] + p.sum_sq, sums[2] + p.sum_err]
        return cls(sum(p.pairs for p in parts), sum(p.estimated for p in parts), sum(p.truth_not_finite for p in parts),
                   [sum(p.by_status[q] for p in parts) for q in range(8)], sums[0], sums[1], sums[2], sum(p.ms for p in parts))


class PreferenceEstimates(_Result):
    """What ``PreparedItemSimilarity.estimate`` returns: one row per asked pair, in the order asked -- (user, item, estimate float32,
    status); the estimate is NaN unless the status is FY_ESTIMATE_OK.  ``estimate_stats`` (fy_itemcf_estimate_stats) beside ``stats``."""

    def __init__(self, handle, ctx=None):
        super().__init__(handle, ctx)
        self.stats = self._stats()
        self.size = self._lib.fy_result_size(handle)
        self._rows = None
        es = _native.ItemCFEstimateStats()
        _check(self._lib.fy_result_itemcf_estimate_stats(handle, C.byref(es)))
        self.estimate_stats = es.as_dict()

    def rows(self):
        if self._rows is None:
            L, h, n = self._lib, self._h, self.size
            self._rows = {"user": _np(L.fy_result_key0(h), n, np.int32), "item": _np(L.fy_result_key1(h), n, np.int32),
                          "estimate": _np(L.fy_result_value(h), n, np.float32), "status": _np(L.fy_result_aux(h), n, np.int32)}
        return self._rows

    def errors(self, truth, clamp=None):
        """fy_eval_estimates: the error sums against ``truth``, a resident ``Ratings`` whose entries (from this result's pair offset
        on) are the asked pairs in the same order -- the ``Ratings`` the estimates were asked for, typically.  ``clamp=(lo, hi)``
        clamps every estimate into the rating scale first.  Returns an ``EstimateErrors``; nothing is downloaded but the sums."""
        p = _native.EvalErrorParams(0, 0, 0.0, 0.0) if clamp is None else _native.EvalErrorParams(1, 0, float(clamp[0]), float(clamp[1]))
        e = _native.EvalErrors()
        _check(self._lib.fy_eval_estimates(self._ctx._h, self._h, truth._h, C.byref(p), C.byref(e)))
        return EstimateErrors(e.pairs, e.estimated, e.truth_not_finite, list(e.by_status), e.sum_abs, e.sum_sq, e.sum_err, e.ms)


class PreferenceExplanations(_Result):
    """What ``PreparedItemSimilarity.because`` returns.  ``rows()``: the listed contributors grouped by asked pair in the order asked,
    best first -- ``pair`` (index of the asked pair inside this rank's range), ``user``, ``item`` (of the asked pair), ``because`` (the
    contributing item), ``sim`` (float32, the job's row entry) and ``pref`` (float32; 1 with booleanData).  ``pairs()``: one entry per
    asked pair -- ``user``, ``item``, ``estimate``, ``status`` (FY_ESTIMATE_*), ``contributors`` (all of them, listed or not) and
    ``start`` (pairs + 1: the rows of pair t are start[t] .. start[t + 1]).  ``because_stats`` (fy_itemcf_because_stats) beside
    ``stats``.  Nothing is computed on the host."""

    def __init__(self, handle, ctx=None):
        super().__init__(handle, ctx)
        self.stats = self._stats()
        self.size = self._lib.fy_result_size(handle)
        self._rows = self._pairs = None
        bs = _native.ItemCFBecauseStats()
        _check(self._lib.fy_result_itemcf_because_stats(handle, C.byref(bs)))
        self.because_stats = bs.as_dict()

    def _view(self):
        v = _native.ItemCFBecauseView()
        _check(self._lib.fy_result_because_view(self._h, C.byref(v)))
        return v

    def pairs(self):
        if self._pairs is None:
            v = self._view()
            n = v.n_pairs
            start = _np(v.start, n + 1, np.int64)
            self._pairs = {"user": _np(v.user, n, np.int32), "item": _np(v.item, n, np.int32), "estimate": _np(v.estimate, n, np.float32),
                           "status": _np(v.status, n, np.int32), "contributors": _np(v.contributors, n, np.int32),
                           "start": start if len(start) else np.zeros(1, dtype=np.int64)}
        return self._pairs

    def rows(self):
        if self._rows is None:
            L, h, n = self._lib, self._h, self.size
            pair = _np(L.fy_result_aux(h), n, np.int32)
            self._rows = {"pair": pair, "user": _np(L.fy_result_key0(h), n, np.int32), "item": self.pairs()["item"][pair],
                          "because": _np(L.fy_result_key1(h), n, np.int32), "sim": _np(L.fy_result_value(h), n, np.float32),
                          "pref": _np(self._view().pref, n, np.float32)}
        return self._rows


class Evaluator:
    """Ranking metrics of list results where they lie in HBM (fy_eval_*; include/filmyou.h states the definitions).

    Prepared once from the ``test`` Ratings (a hold-out, ``Ratings.holdout``): a test entry is relevant iff its score is
    >= ``relevance_threshold``; ``gain`` = ``binary`` (1), ``linear`` (the score) or ``exp2`` (2^score - 1) for nDCG; ``cutoffs``
    strictly ascending, each at most 4096; ``coverage`` also counts the distinct items recommended.  ``test`` may be closed
    afterwards."""

    GAIN = {"binary": 0, "linear": 1, "exp2": 2}

    def __init__(self, ctx, test, cutoffs=(10,), relevance_threshold=4.0, gain="binary", coverage=False):
        self._lib = _native.load()
        self._ctx = ctx
        self._h = None
        if gain not in self.GAIN:
            raise ValueError("gain must be binary, linear or exp2 (got %r)" % (gain,))
        cutoffs = tuple(int(c) for c in cutoffs)
        if not 1 <= len(cutoffs) <= 8:
            raise ValueError("1 to 8 cutoffs")
        p = _native.EvalParams(len(cutoffs), (C.c_int32 * 8)(*cutoffs), self.GAIN[gain], 1 if coverage else 0, float(relevance_threshold))
        h = C.c_void_p()
        _check(self._lib.fy_eval_prepare(ctx._h, C.byref(p), test._h, C.byref(h)))
        self._h = h
        self.cutoffs = cutoffs

    def evaluate(self, result, per_user=False):
        """fy_eval_lists on a ``Recommendations`` or ``ItemRecommendations`` of this evaluator's context.  Returns an ``Evaluation``."""
        s = _native.EvalSums()
        ids = vals = None
        if per_user:
            # `lists` is at most the result's row count; a first call without the arrays says how many there are
            _check(self._lib.fy_eval_lists(self._h, result._h, C.byref(s), None, None))
            ids = np.empty(s.lists, dtype=np.int32)
            vals = np.empty((s.lists, len(self.cutoffs), 5), dtype=np.float64)
        _check(self._lib.fy_eval_lists(self._h, result._h, C.byref(s), ids.ctypes.data if per_user else None,
                                       vals.ctypes.data if per_user else None))
        n = s.n_cutoffs
        pu = None
        if per_user:
            pu = {"user": ids, "hits": vals[:, :, 0], "recall": vals[:, :, 1], "ap": vals[:, :, 2], "rr": vals[:, :, 3], "ndcg": vals[:, :, 4]}
        return Evaluation(list(s.cutoffs)[:n], {k: getattr(s, k) for k in Evaluation.COUNTERS}, list(s.hits)[:n], list(s.users_hit)[:n],
                          {k: list(getattr(s, k))[:n] for k in Evaluation.SUMS}, s.distinct_items if s.distinct_items >= 0 else None, s.ms, pu)

    def close(self):
        if getattr(self, "_h", None):
            if self._ctx._h:
                self._lib.fy_eval_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BaselineRecommenderJob:
    """Item-based CF (M/baselinerecommender/BaselineRecommenderJob.java:179-328) from the similarity phase on: phase 2
    (RowSimilarityJob), phase 3 (partialMultiply) and phase 4 (aggregateAndRecommend) on the GPU, with the job's
    option names and defaults (:140-176)."""

    JOB_NAME = "BaselineRecommenderJob"

    def __init__(self, ctx=None):
        self.ctx = ctx

    def prepare(self, ratings, maxSimilaritiesPerItem=100, similarityClassname=SIMILARITY_COSINE, threshold=None, ratingShift=0.0):
        """The similarity phase of ``run`` as a prepared job: a ``PreparedItemSimilarity`` whose ``recommend(users)`` answers
        "these users just rated something" without building the similarity matrix.  The options are those ``run`` passes to
        phase 2: self-similarity excluded, world 1, no input preparation, ratingShift applied first.  ``ratings`` (a ``Ratings``
        or a triple of arrays) may be closed afterwards; after a write, prepare again on the new ``Ratings``."""
        ctx = self.ctx or Context(0)
        self.ctx = ctx
        own_ratings = not isinstance(ratings, Ratings)
        r = Ratings(ctx, *ratings) if own_ratings else ratings
        if float(ratingShift) != 0.0:
            try:
                shifted = r.shifted(ratingShift)
            finally:
                if own_ratings:
                    r.close()
            r, own_ratings = shifted, True
        try:
            try:
                return RowSimilarityJob(ctx).prepare(r, similarityClassname, maxSimilaritiesPerItem, True, threshold)
            except RuntimeError as e:      # the similarity phase's failure under this job's name
                if isinstance(e.__cause__, FilmYouError):
                    raise RuntimeError("%s failed!: %s" % (self.JOB_NAME, e.__cause__.message)) from e.__cause__
                raise
        finally:
            if own_ratings:
                r.close()

    def run(self, ratings, numRecommendations=100, maxPrefsPerUser=50, maxSimilaritiesPerItem=100,
            similarityClassname=SIMILARITY_COSINE, threshold=None, booleanData=False, rank=0, world=1,
            similarities=None, usersFile=None, itemsFile=None, ratingShift=0.0, outputPathForSimilarityMatrix=None):
        """Returns (ItemRecommendations, ItemSimilarities).  `similarities` may be passed to skip phase 2
        (Mahout's --startPhase).

        usersFile / itemsFile (a path of one id per line, or an integer array; None = not given): lists only for these users
        (BaselineRecommenderJob.java:305-307), only these items may be recommended (BaselineAggregateAndRecommendReducer.java:170-181,
        209) -- fy_itemcf_recommend_filtered, whose cost follows the users asked for.  ratingShift: every preference is
        float32(score + ratingShift) for the similarity build and the recommendation pass alike (BaselineToItemPrefsMapper.java:60).
        outputPathForSimilarityMatrix: the similarity matrix is also written there as de-duplicated item pairs, text
        (BaselineRecommenderJob.java:259-278)."""
        lib = _native.load()
        ctx = self.ctx or Context(0)
        self.ctx = ctx
        users, items = _id_list(usersFile), _id_list(itemsFile)
        own_ratings = not isinstance(ratings, Ratings)
        r = Ratings(ctx, *ratings) if own_ratings else ratings
        if float(ratingShift) != 0.0:
            try:
                shifted = r.shifted(ratingShift)
            finally:
                if own_ratings:
                    r.close()
            r, own_ratings = shifted, True
        try:
            sims = similarities
            if sims is None:
                # every rank needs the whole matrix for phase 3: built with world = 1
                sims = RowSimilarityJob(ctx).run(r, similarityClassname, maxSimilaritiesPerItem, True, threshold)
            p = _native.ItemCFParams(int(numRecommendations), int(maxPrefsPerUser), 1 if booleanData else 0, int(rank),
                                     int(world), 0)
            if outputPathForSimilarityMatrix is not None:
                write_similarity_pairs(outputPathForSimilarityMatrix, sims.pairs())
            res = C.c_void_p()
            try:
                ctx.sync_tuning()
                if users is None and items is None:
                    _check(lib.fy_itemcf_recommend(ctx._h, C.byref(p), r._h, sims._h, C.byref(res)))
                else:
                    f = _native.ItemCFFilter(int(users is not None), int(items is not None),
                                             0 if users is None else len(users), None if users is None else users.ctypes.data,
                                             0 if items is None else len(items), None if items is None else items.ctypes.data)
                    _check(lib.fy_itemcf_recommend_filtered(ctx._h, C.byref(p), C.byref(f), r._h, sims._h, C.byref(res)))
            except FilmYouError as e:
                raise RuntimeError("%s failed!: %s" % (self.JOB_NAME, e.message)) from e
            return ItemRecommendations(res, ctx), sims
        finally:
            if own_ratings:
                r.close()


class RowSimilarityJob:
    """Item-item similarity build with the options the reference passes to Mahout's RowSimilarityJob
    (M/baselinerecommender/BaselineRecommenderJob.java:241-253)."""

    JOB_NAME = "RowSimilarityJob"

    def __init__(self, ctx=None):
        self.ctx = ctx

    @staticmethod
    def _params(similarityClassname, maxSimilaritiesPerRow, excludeSelfSimilarity, threshold, rank, world, minPrefsPerUser, maxPrefsPerUser):
        return _native.ItemSimParams(similarity_id(similarityClassname), int(maxSimilaritiesPerRow),
                                     1 if excludeSelfSimilarity else 0, 0 if threshold is None else 1,
                                     0.0 if threshold is None else float(threshold), int(rank), int(world), 0,
                                     int(minPrefsPerUser), 0 if maxPrefsPerUser is None else int(maxPrefsPerUser))

    def prepare(self, ratings, similarityClassname=SIMILARITY_COSINE, maxSimilaritiesPerRow=100,
                excludeSelfSimilarity=True, threshold=None, rank=0, world=1, minPrefsPerUser=1, maxPrefsPerUser=None):
        """fy_itemsim_prepare: everything the job derives from the ratings and these options alone, once (O(nnz)); the options
        mean what they mean for ``run``.  Returns a ``PreparedItemSimilarity`` whose ``rows(ids)`` answers requests for the
        rows of named items.  ``ratings`` (a ``Ratings`` or a triple of arrays) may be closed afterwards."""
        lib = _native.load()
        p = self._params(similarityClassname, maxSimilaritiesPerRow, excludeSelfSimilarity, threshold, rank, world, minPrefsPerUser,
                         maxPrefsPerUser)
        ctx = self.ctx or Context(0)
        self.ctx = ctx
        own_ratings = not isinstance(ratings, Ratings)
        r = Ratings(ctx, *ratings) if own_ratings else ratings
        job = C.c_void_p()
        try:
            try:
                ctx.sync_tuning()
                _check(lib.fy_itemsim_prepare(ctx._h, C.byref(p), r._h, C.byref(job)))
            except FilmYouError as e:
                raise RuntimeError("%s failed!: %s" % (self.JOB_NAME, e.message)) from e
            return PreparedItemSimilarity(job, ctx)
        finally:
            if own_ratings:
                r.close()

    def run(self, ratings, similarityClassname=SIMILARITY_COSINE, maxSimilaritiesPerRow=100,
            excludeSelfSimilarity=True, threshold=None, rank=0, world=1, minPrefsPerUser=1, maxPrefsPerUser=None, itemsFile=None):
        """minPrefsPerUser / maxPrefsPerUser: the input preparation in front of the similarity job
        (BaselinePreparePreferenceMatrixJob.java:104, 126-129).  Users with fewer preferences than minPrefsPerUser are
        dropped (reference default 1).  maxPrefsPerUser = the reference's maxPrefsPerUserInItemSimilarity (its default 1000 draws
        a RANDOM sample in Mahout's ToItemVectorsMapper); here None = no cap, a number = a DETERMINISTIC systematic sample
        (include/filmyou.h) -- no parity with any particular Mahout run.
        itemsFile: a path of one item id per line (read_id_file) or an integer array: the rows of these items alone, with the
        work sized by the request (prepare + PreparedItemSimilarity.rows); None = the whole matrix."""
        if itemsFile is not None:
            # read before any device work (an array goes to rows() as it is: ids outside int32 are dropped there, not wrapped)
            items = read_id_file(itemsFile) if isinstance(itemsFile, (str, bytes, os.PathLike)) else np.asarray(itemsFile)
            prepared = self.prepare(ratings, similarityClassname, maxSimilaritiesPerRow, excludeSelfSimilarity, threshold, rank, world,
                                    minPrefsPerUser, maxPrefsPerUser)
            try:
                return prepared.rows(items)
            finally:
                prepared.close()
        lib = _native.load()
        p = self._params(similarityClassname, maxSimilaritiesPerRow, excludeSelfSimilarity, threshold, rank, world, minPrefsPerUser,
                         maxPrefsPerUser)
        ctx = self.ctx or Context(0)
        self.ctx = ctx
        own_ratings = not isinstance(ratings, Ratings)
        r = Ratings(ctx, *ratings) if own_ratings else ratings
        res = C.c_void_p()
        try:
            try:
                ctx.sync_tuning()
                _check(lib.fy_itemsim_build(ctx._h, C.byref(p), r._h, C.byref(res)))
            except FilmYouError as e:
                raise RuntimeError("%s failed!: %s" % (self.JOB_NAME, e.message)) from e
            return ItemSimilarities(res, ctx)
        finally:
            if own_ratings:
                r.close()


class PreparedItemSimilarity:
    """A prepared item-similarity job (fy_itemsim_job): the structure of the ratings, the per-item norms and the request
    kernel's row offsets are in HBM; the ratings object it was made from is no longer needed."""

    def __init__(self, handle, ctx):
        self._lib = _native.load()
        self._h = handle
        self._ctx = ctx

    def rows(self, ids):
        """fy_itemsim_rows: the rows the full build would emit for the listed raw item ids (any order, duplicates and unknown
        ids passed over), with the work sized by the request.  Any number of calls; the job stays as it was.  Returns an
        ``ItemSimilarities`` with ``request_stats`` beside ``stats``."""
        ids = np.asarray(ids).reshape(-1)
        if ids.dtype != np.int32:      # an id outside int32 is outside the data: passed over, never wrapped into range (as read_id_file does)
            ids = np.asarray(ids, dtype=np.int64) if len(ids) else np.zeros(0, dtype=np.int64)
            ids = ids[(ids >= -2 ** 31) & (ids < 2 ** 31)]
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        rq = _native.ItemSimRequest(len(ids), ids.ctypes.data if len(ids) else None)
        res = C.c_void_p()
        try:
            self._ctx.sync_tuning()
            _check(self._lib.fy_itemsim_rows(self._h, C.byref(rq), C.byref(res)))
        except FilmYouError as e:
            raise RuntimeError("%s failed!: %s" % (RowSimilarityJob.JOB_NAME, e.message)) from e
        return ItemSimilarities(res, self._ctx, request=True)

    def recommend(self, users, numRecommendations=100, maxPrefsPerUser=50, booleanData=False, itemsFile=None, rank=0, world=1):
        """fy_itemcf_recommend_prepared: the lists ``BaselineRecommenderJob.run(usersFile=users)`` would emit on the ratings this
        job was prepared on, from the similarity rows of the users' own strongest preferences alone.  Rows built by a call stay
        on the job for later calls (``drop_rows`` releases them); they change no result.  ``users`` / ``itemsFile``: a path of
        one id per line or an integer array.  Returns an ``ItemRecommendations`` with ``request_stats`` beside ``stats``."""
        if users is None:
            raise ValueError("recommend() needs the users to recommend for; BaselineRecommenderJob.run serves every user")
        users, items = _id_list(users), _id_list(itemsFile)
        p = _native.ItemCFParams(int(numRecommendations), int(maxPrefsPerUser), 1 if booleanData else 0, int(rank), int(world), 0)
        f = _native.ItemCFFilter(1, int(items is not None), len(users), users.ctypes.data if len(users) else None,
                                 0 if items is None else len(items), None if items is None or not len(items) else items.ctypes.data)
        res = C.c_void_p()
        try:
            self._ctx.sync_tuning()
            _check(self._lib.fy_itemcf_recommend_prepared(self._h, C.byref(p), C.byref(f), C.byref(res)))
        except FilmYouError as e:
            raise RuntimeError("%s failed!: %s" % (BaselineRecommenderJob.JOB_NAME, e.message)) from e
        return ItemRecommendations(res, self._ctx, request=True)

    def recommend_profiles(self, profiles, numRecommendations=100, maxPrefsPerUser=50, booleanData=False, itemsFile=None, base="whole",
                           ratingShift=0.0, rank=0, world=1):
        """fy_itemcf_recommend_profiles: the lists of ``recommend`` for preference vectors handed in -- an anonymous or new user's whole
        profile (``base="whole"``), or a resident user's row of the prepared ratings with pending writes applied
        (``base="resident"``: the label is the user id) -- on the standing job and its warm row store, without preparing again.  The
        similarity rows stay as prepared.  ``profiles``: a sequence of ``(label, items, scores)`` / ``(label, items, scores,
        remove)``, or the CSR arrays ``(labels, start, item, score[, remove])`` as a tuple of numpy arrays.  Per profile the last
        entry of an item counts, a non-zero ``remove`` deletes the item, an item nobody rated in the prepared ratings is dropped
        (include/filmyou.h states the rules).  ``ratingShift``: every given score becomes float32(score + shift) first, so a job
        prepared with a ratingShift is fed raw scores.  Rows are grouped by profile in the order given, labelled ``label``; (rank,
        world) cut the profile list.  Returns an ``ItemRecommendations`` with ``profile_stats`` beside ``stats``."""
        if profiles is None:
            raise ValueError("recommend_profiles() needs the profiles to recommend for")
        q, keep = _itemcf_profiles(profiles, base, float(ratingShift))
        items = _id_list(itemsFile)
        p = _native.ItemCFParams(int(numRecommendations), int(maxPrefsPerUser), 1 if booleanData else 0, int(rank), int(world), 0)
        f = _native.ItemCFFilter(0, int(items is not None), 0, None, 0 if items is None else len(items),
                                 None if items is None or not len(items) else items.ctypes.data)
        res = C.c_void_p()
        try:
            self._ctx.sync_tuning()
            _check(self._lib.fy_itemcf_recommend_profiles(self._h, C.byref(p), C.byref(q), C.byref(f), C.byref(res)))
            del keep
        except FilmYouError as e:
            raise RuntimeError("%s failed!: %s" % (BaselineRecommenderJob.JOB_NAME, e.message)) from e
        return ItemRecommendations(res, self._ctx, request="profiles")

    def estimate(self, pairs, maxPrefsPerUser=50, booleanData=False, rank=0, world=1):
        """fy_itemcf_estimate_prepared / fy_itemcf_estimate_ratings: what would this user give this item -- the cell (user, item) of
        the pass ``recommend`` runs, before the top-N (bit for bit the list's score wherever a list holds the pair), with the work
        sized by the pairs.  ``pairs``: ``(users, items)`` raw-id arrays (numpy, or int32 torch tensors on the context's GPU), or a
        resident ``Ratings`` whose (user, item) columns are asked in its order (the ``test`` side of ``Ratings.holdout``: no id
        leaves the GPU).  (rank, world) cut the pair list.  Rows built stay on the job like ``recommend``'s.  Returns a
        ``PreferenceEstimates``."""
        p = _native.ItemCFParams(0, int(maxPrefsPerUser), 1 if booleanData else 0, int(rank), int(world), 0)
        res = C.c_void_p()
        try:
            self._ctx.sync_tuning()
            if isinstance(pairs, Ratings):
                _check(self._lib.fy_itemcf_estimate_ratings(self._h, C.byref(p), pairs._h, C.byref(res)))
            else:
                q, keep = _itemcf_pairs(pairs)
                _check(self._lib.fy_itemcf_estimate_prepared(self._h, C.byref(p), C.byref(q), C.byref(res)))
                del keep
        except FilmYouError as e:
            raise RuntimeError("%s failed!: %s" % (BaselineRecommenderJob.JOB_NAME, e.message)) from e
        return PreferenceEstimates(res, self._ctx)

    def because(self, pairs, howMany=5, maxPrefsPerUser=50, booleanData=False, rank=0, world=1):
        """fy_itemcf_because_prepared: "because you liked ..." -- for every asked pair the kept preferences of the user whose
        similarity rows hold the item, i.e. the terms of the sum ``estimate`` finishes for the same pair, the ``howMany`` (1 .. 64)
        heaviest listed (weight pref * sim descending, equal weights by ascending item id, NaN last), with the pair's estimate, status
        and count of contributors bit for bit ``estimate``'s.  ``pairs``: ``(users, items)`` raw-id arrays (numpy, or int32 torch
        tensors on the context's GPU).  (rank, world) cut the pair list.  Rows built stay on the job like ``recommend``'s.  Returns
        a ``PreferenceExplanations``."""
        p = _native.ItemCFParams(0, int(maxPrefsPerUser), 1 if booleanData else 0, int(rank), int(world), 0)
        res = C.c_void_p()
        try:
            self._ctx.sync_tuning()
            q, keep = _itemcf_pairs(pairs)
            _check(self._lib.fy_itemcf_because_prepared(self._h, C.byref(p), C.byref(q), int(howMany), C.byref(res)))
            del keep
        except FilmYouError as e:
            raise RuntimeError("%s failed!: %s" % (BaselineRecommenderJob.JOB_NAME, e.message)) from e
        return PreferenceExplanations(res, self._ctx)

    def drop_rows(self):
        """fy_itemsim_job_drop_rows: releases the similarity rows kept by ``recommend``; the job stays valid."""
        if getattr(self, "_h", None) and self._ctx._h:
            self._lib.fy_itemsim_job_drop_rows(self._h)

    def close(self):
        if getattr(self, "_h", None):
            if self._ctx._h:
                self._lib.fy_itemsim_job_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ClusterAssignmentJob:
    """Cluster assignment in front of the RM2 job (M/nmf/clustering/ClusterAssignmentJob.java:60-135 + CountClustersJob):
    every user goes to the cluster of the largest entry of its row of H (FindClusterMapper.java:37-45), or -- sub-clustering,
    FindSubClusterMapper.java:46-76 -- to  parent * ceil(numberOfUsers / numberOfClusters) + argmax  of its row of that
    parent cluster's H.  ``run`` returns ``(users, clusters, counts)``: the reference's `clustering` and `clusteringCount`
    files as arrays, i.e. the ``clustering=(users, clusters), clustering_count=counts`` arguments of ``RM2Job.run``."""

    def __init__(self, context):
        self._ctx = context
        self._lib = _native.load()

    def _assign(self, H, first_user, offset, counts):
        import numpy as np
        device = hasattr(H, "is_cuda") and H.is_cuda
        if device:
            import torch
            assert H.dtype == torch.float64 and H.is_contiguous() and H.dim() == 2
            torch.cuda.current_stream(H.device).synchronize()
            n, k, ptr = int(H.shape[0]), int(H.shape[1]), H.data_ptr()
        else:
            H = np.ascontiguousarray(H, dtype=np.float64)
            if H.ndim != 2:
                raise ValueError("H must be a (users x clusters) matrix")
            n, k, ptr = H.shape[0], H.shape[1], H.ctypes.data
        users, clusters = np.zeros(n, np.int32), np.zeros(n, np.int32)
        _check(self._lib.fy_cluster_assign(self._ctx._h, n, k, ptr, 1 if device else 0, int(first_user),
                                           int(offset), len(counts), users.ctypes.data, clusters.ctypes.data,
                                           counts.ctypes.data if len(counts) else None))
        return users, clusters

    def run(self, H, first_user=1, number_of_clusters=None):
        """H: (users x numberOfClusters) float64, numpy or a CUDA torch tensor.  first_user: id of row 0 (the reference's H
        files are keyed from 1)."""
        import numpy as np
        if len(H.shape) != 2:
            raise ValueError("H must be a (users x clusters) matrix")
        k = int(H.shape[1]) if number_of_clusters is None else int(number_of_clusters)
        counts = np.zeros(k, np.int32)
        users, clusters = self._assign(H, first_user, 0, counts)
        return users, clusters, counts

    def run_sub(self, parts, number_of_users, number_of_clusters):
        """Sub-clustering: parts = [(parent_cluster, H_parent, first_user), ...] (one H per `cluster<c>` directory of the
        reference); the total number of clusters becomes numberOfClusters * ceil(numberOfUsers / numberOfClusters)."""
        import numpy as np
        n_sub = -(-int(number_of_users) // int(number_of_clusters))
        counts = np.zeros(n_sub * int(number_of_clusters), np.int32)
        us, cs = [], []
        for parent, H, first_user in parts:
            u, c = self._assign(H, first_user, int(parent) * n_sub, counts)
            us.append(u)
            cs.append(c)
        return np.concatenate(us), np.concatenate(cs), counts


class NMFDriver:
    """NMF (``ppc=False``, M/nmf/NMFDriver.java) or PPC (``ppc=True``, M/nmf/ppc/PPCDriver.java) factorisation of the rating
    matrix: ``run`` performs numberOfIterations multiplicative updates of (H, W) (M/nmf/AbstractNMFDriver.java:118-146) on the
    GPU in fp64 and returns the new ``(H, W)``.  H is (numberOfUsers x numberOfClusters), W (numberOfItems x numberOfClusters);
    row r belongs to id r + 1.  Configuration keys: numberOfUsers, numberOfItems, numberOfClusters, numberOfIterations,
    normalizationFrequency (PPC; Java's ``iteration % f``; 0 = never)."""

    def __init__(self, conf, context, ppc=False):
        self._conf, self._ctx, self._ppc = conf, context, bool(ppc)
        self._lib = _native.load()
        self.stats = None

    def run(self, ratings, H, W):
        import numpy as np
        conf = self._conf
        H = np.array(H, dtype=np.float64, order="C")
        W = np.array(W, dtype=np.float64, order="C")
        n_users = conf.getInt("numberOfUsers", H.shape[0])
        n_items = conf.getInt("numberOfItems", W.shape[0])
        k = conf.getInt("numberOfClusters", H.shape[1])
        if H.shape != (n_users, k) or W.shape != (n_items, k):
            raise ValueError("H must be numberOfUsers x numberOfClusters and W numberOfItems x numberOfClusters")
        p = _native.NMFParams(n_users, n_items, k, conf.getInt("numberOfIterations", 1), 1 if self._ppc else 0,
                              conf.getInt("normalizationFrequency", -1))
        own = not isinstance(ratings, Ratings)
        r = Ratings(self._ctx, *ratings) if own else ratings
        try:
            st = _native.Stats()
            try:
                _check(self._lib.fy_nmf_factorize(self._ctx._h, C.byref(p), r._h, H.ctypes.data, W.ctypes.data, C.byref(st)))
            except FilmYouError as e:
                raise RuntimeError("%s failed!: %s" % ("PPC" if self._ppc else "NMF", e.message)) from e
            self.stats = st.as_dict()
        finally:
            if own:
                r.close()
        return H, W


class SubClusterMappings:
    """What SubClusterMappingJob leaves behind (the reference's `mapping/<cluster>` and `subClustering{User,Item}/clusteringCount`
    files), as arrays.  Users and items come cluster after cluster, inside a cluster by ascending raw id; `*_new_id` counts from 1
    inside the cluster.  ``csr`` / ``csc``: the kept ratings over these rows, ``(rowptr, col, value)`` with ``col`` a row of the
    other side."""

    def __init__(self, lib, h, n_clusters):
        i32 = np.int32
        nu, ni, nnz = lib.fy_submap_n_users(h), lib.fy_submap_n_items(h), lib.fy_submap_nnz(h)
        self.users_in_cluster, self.items_in_cluster = np.zeros(n_clusters, i32), np.zeros(n_clusters, i32)
        _check(lib.fy_submap_counts(h, self.users_in_cluster.ctypes.data, self.items_in_cluster.ctypes.data))
        self.user, self.user_cluster, self.user_new_id = np.zeros(nu, i32), np.zeros(nu, i32), np.zeros(nu, i32)
        _check(lib.fy_submap_users(h, self.user.ctypes.data, self.user_cluster.ctypes.data, self.user_new_id.ctypes.data))
        self.item, self.item_cluster, self.item_new_id = np.zeros(ni, i32), np.zeros(ni, i32), np.zeros(ni, i32)
        _check(lib.fy_submap_items(h, self.item.ctypes.data, self.item_cluster.ctypes.data, self.item_new_id.ctypes.data))
        self.nnz = nnz
        self.csr = (np.zeros(nu + 1, i32), np.zeros(nnz, i32), np.zeros(nnz, np.float32))
        self.csc = (np.zeros(ni + 1, i32), np.zeros(nnz, i32), np.zeros(nnz, np.float32))
        for by_item, (p, c, v) in ((0, self.csr), (1, self.csc)):
            _check(lib.fy_submap_matrix(h, by_item, p.ctypes.data, c.ctypes.data, v.ctypes.data))


def _clustering_arrays(clustering):
    mu, mc = (_i32(clustering[0]), _i32(clustering[1])) if clustering is not None else (_i32(None), _i32(None))
    if len(mu) != len(mc):
        raise ValueError("clustering users / clusters differ in length")
    return mu, mc


class SubClusterMappingJob:
    """New user and item ids per parent cluster (M/nmf/clustering/SubClusterMappingJob.java with User / ItemMappingReducer),
    for all parent clusters in one pass on the GPU.  Configuration key: numberOfClusters.  The order of the new ids, which the
    reference leaves to the shuffle, is ascending raw id."""

    JOB_NAME = "SubClusterMappingJob"

    def __init__(self, conf, context):
        self._conf, self._ctx = conf, context
        self._lib = _native.load()

    def run(self, ratings, clustering):
        """ratings: a ``Ratings`` or a (user, item, score) triple; clustering: (users, clusters) of the parent clustering."""
        K = self._conf.getInt("numberOfClusters", -1)
        if K is None or K <= 0:
            raise ValueError("Invalid number of clusters (%s)" % K)      # RMRecommenderDriver.java:302-305
        mu, mc = _clustering_arrays(clustering)
        own = not isinstance(ratings, Ratings)
        r = Ratings(self._ctx, *ratings) if own else ratings
        h = C.c_void_p()
        try:
            try:
                _check(self._lib.fy_submap_create(self._ctx._h, r._h, K, len(mu), mu.ctypes.data, mc.ctypes.data, C.byref(h)))
                return SubClusterMappings(self._lib, h, K)
            except FilmYouError as e:
                raise RuntimeError("%s failed!: %s" % (self.JOB_NAME, e.message)) from e
        finally:
            if h:
                self._lib.fy_submap_destroy(h)
            if own:
                r.close()


class ClusterRefinementJob:
    """Cluster refinement (RMRecommenderDriver.clusterRefinement, M/rmrecommender/RMRecommenderDriver.java:217-266): the
    mappings, one PPC (``ppc=True``, what the reference runs) or NMF factorisation per parent cluster with
    ceil(usersInCluster / usersPerSubCluster) sub-clusters, and ClusterAssignmentJob(true) -- all parent clusters in one batched
    pass on the GPU (fy_cluster_refine).  Configuration keys: numberOfUsers (only the id stride
    ceil(numberOfUsers / numberOfClusters)), numberOfClusters, usersPerSubCluster, numberOfIterations, normalizationFrequency
    (unset = -1, like NMFDriver).  ``run`` returns ``(users, clusters, counts)`` like ``ClusterAssignmentJob.run_sub``;
    afterwards ``stats`` (fy_refine_stats), ``users_in_cluster`` / ``items_in_cluster`` / ``sub_clusters`` per parent and, with
    ``keep_factors=True``, ``factors`` = [(H_c, W_c), ...] per parent are set."""

    JOB_NAME = "ClusterRefinement"

    def __init__(self, conf, context, ppc=True):
        self._conf, self._ctx, self._ppc = conf, context, bool(ppc)
        self._lib = _native.load()
        self.stats = self.factors = self.users_in_cluster = self.items_in_cluster = self.sub_clusters = None

    def run(self, ratings, clustering, H0=None, W0=None, seed=0, keep_factors=False):
        """H0 / W0: the initial matrices, either a list with one (n_c x k_c) / (m_c x k_c) array per parent cluster (rows in
        new-id order = ascending raw id) or the concatenated flat array; None: the device draws them from ``seed``
        (include/filmyou.h gives the formula)."""
        conf = self._conf
        K, ups = conf.getInt("numberOfClusters", -1), conf.getInt("usersPerSubCluster", -1)
        n_users = conf.getInt("numberOfUsers", -1)
        if K is None or K <= 0:
            raise ValueError("Invalid number of clusters (%s)" % K)
        if ups is None or ups <= 0:
            raise ValueError("usersPerSubCluster must be > 0 (%s)" % ups)
        if n_users is None or n_users <= 0:
            raise ValueError("numberOfUsers is required")
        if (H0 is None) != (W0 is None):
            raise ValueError("H0 and W0 must be given together")
        mu, mc = _clustering_arrays(clustering)

        def flat(M):
            if isinstance(M, (list, tuple)):
                M = np.concatenate([np.asarray(m, dtype=np.float64).ravel() for m in M]) if len(M) else np.zeros(0)
            return np.ascontiguousarray(M, dtype=np.float64).ravel()
        p = _native.RefineParams(n_users, K, ups, conf.getInt("numberOfIterations", 1), 1 if self._ppc else 0,
                                 conf.getInt("normalizationFrequency", -1), int(seed) & 0xFFFFFFFFFFFFFFFF)
        own = not isinstance(ratings, Ratings)
        r = Ratings(self._ctx, *ratings) if own else ratings
        h = C.c_void_p()
        lib = self._lib
        try:
            h0, w0 = (flat(H0), flat(W0)) if H0 is not None else (None, None)
            if h0 is not None:
                # the sizes are known only after the mappings: the library reads sum n_c k_c / sum m_c k_c doubles, so check first
                m = SubClusterMappingJob(conf, self._ctx).run(r, (mu, mc))
                kc = -(-m.users_in_cluster.astype(np.int64) // ups)
                if len(h0) != int((m.users_in_cluster * kc).sum()) or len(w0) != int((m.items_in_cluster * kc).sum()):
                    raise ValueError("H0 / W0 must hold usersInCluster x subClusters and itemsInCluster x subClusters values per parent cluster")
            try:
                _check(lib.fy_cluster_refine(self._ctx._h, C.byref(p), r._h, len(mu), mu.ctypes.data, mc.ctypes.data,
                                             h0.ctypes.data if h0 is not None else None, w0.ctypes.data if w0 is not None else None,
                                             C.byref(h)))
            except FilmYouError as e:
                raise RuntimeError("%s failed!: %s" % (self.JOB_NAME, e.message)) from e
            n, nc = lib.fy_refined_n_users(h), lib.fy_refined_n_counts(h)
            users, clusters, counts = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(nc, np.int32)
            _check(lib.fy_refined_clustering(h, users.ctypes.data, clusters.ctypes.data, counts.ctypes.data))
            nu, ni, kc = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.int32)
            _check(lib.fy_refined_layout(h, nu.ctypes.data, ni.ctypes.data, kc.ctypes.data))
            self.users_in_cluster, self.items_in_cluster, self.sub_clusters = nu, ni, kc
            st = _native.RefineStats()
            _check(lib.fy_refined_stats(h, C.byref(st)))
            self.stats = st.as_dict()
            self.factors = None
            if keep_factors:
                H, W = np.zeros(lib.fy_refined_h_size(h)), np.zeros(lib.fy_refined_w_size(h))
                _check(lib.fy_refined_factors(h, H.ctypes.data, W.ctypes.data))
                ho = np.r_[0, np.cumsum(nu.astype(np.int64) * kc)]
                wo = np.r_[0, np.cumsum(ni.astype(np.int64) * kc)]
                self.factors = [(H[ho[c]:ho[c + 1]].reshape(nu[c], kc[c]), W[wo[c]:wo[c + 1]].reshape(ni[c], kc[c])) for c in range(K)]
            return users, clusters, counts
        finally:
            if h:
                lib.fy_refined_free(h)
            if own:
                r.close()


class FoldInAssignment:
    """What ``FoldIn.assign`` returns, for this rank's profiles in the order given: ``labels``, ``clusters`` (-1 unless the status is
    FY_FOLDIN_OK), ``parents`` (the top-level argmax; -1 with EMPTY and NO_CLUSTER), ``status`` (FY_FOLDIN_*), ``foldin_stats``
    (fy_foldin_stats as a dict); ``factors()`` downloads the top-level rows (n x k), ``sub_factors()`` the second-level rows as a list
    with one array of k_c values per profile (empty where level 2 did not run)."""

    def __init__(self, handle, k, ctx):
        lib = self._lib = _native.load()
        self._h, self._k = handle, int(k)
        self._ctx = ctx   # the factor rows are downloaded through the context's stream: keep it alive
        n = lib.fy_foldin_result_n(handle)
        self.labels, self.clusters, self.parents, self.status = (np.zeros(n, np.int32) for _ in range(4))
        _check(lib.fy_foldin_result_assignment(handle, self.labels.ctypes.data, self.clusters.ctypes.data, self.parents.ctypes.data,
                                               self.status.ctypes.data))
        st = _native.FoldInStats()
        _check(lib.fy_foldin_result_stats(handle, C.byref(st)))
        self.foldin_stats = st.as_dict()

    def factors(self):
        H = np.zeros((len(self.labels), self._k))
        _check(self._lib.fy_foldin_result_factors(self._h, H.ctypes.data))
        return H

    def sub_factors(self):
        off = np.zeros(len(self.labels) + 1, np.int64)
        H = np.zeros(self._lib.fy_foldin_result_sub_size(self._h))
        _check(self._lib.fy_foldin_result_sub_factors(self._h, off.ctypes.data, H.ctypes.data if len(H) else None))
        return [H[off[p]:off[p + 1]] for p in range(len(self.labels))]

    def close(self):
        if getattr(self, "_h", None):
            if self._ctx._h:      # a result must not outlive its context's stream
                self._lib.fy_foldin_result_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FoldIn:
    """Fold-in of given profiles on standing factors (fy_foldin_*): the item factors ``W`` (numberOfItems x k, row r
    = item id r + 1; numpy or a CUDA float64 torch tensor) of the last PPC (``ppc=True``) / NMF run are held fixed, the reference's H
    update runs for the given rows alone and the cluster is the argmax -- the ``clusters=`` of ``PreparedRM2.score_profiles(base="whole")``
    for a visitor nobody has seen, without a factorisation and without a prepare.  ``counts``: a `clusteringCount`; a cluster without
    resident users cannot win.  ``add_level`` adds the refined level of ``ClusterRefinementJob``.  Only whole profiles are taken: a
    resident row with pending writes is composed by the caller (``Ratings.to_host``)."""

    def __init__(self, ctx, W, ppc=True, normalizationFrequency=-1, counts=None):
        self._ctx, self._lib = ctx, _native.load()
        self._h = C.c_void_p()
        device = hasattr(W, "is_cuda") and W.is_cuda
        if device:
            import torch
            assert W.dtype == torch.float64 and W.is_contiguous() and W.dim() == 2
            torch.cuda.current_stream(W.device).synchronize()
            ptr = W.data_ptr()
        else:
            W = np.ascontiguousarray(W, dtype=np.float64)
            if W.ndim != 2:
                raise ValueError("W must be a (numberOfItems x numberOfClusters) matrix")
            ptr = W.ctypes.data
        self.number_of_items, self.k = int(W.shape[0]), int(W.shape[1])
        p = _native.FoldInParams(self.number_of_items, self.k, 1 if ppc else 0, int(normalizationFrequency))
        cnt = None if counts is None else _i32(counts)
        _check(self._lib.fy_foldin_create(ctx._h, C.byref(p), ptr, 1 if device else 0, cnt.ctypes.data if cnt is not None and len(cnt) else None,
                                          len(cnt) if cnt is not None else 0, C.byref(self._h)))

    def add_level(self, mappings, factors_W, stride, counts=None):
        """mappings: the ``SubClusterMappings`` of the parent clustering; factors_W: one (itemsInCluster x subClusters) array per parent
        (or the ``(H_c, W_c)`` pairs of ``ClusterRefinementJob(...).factors``); stride = ceil(numberOfUsers / numberOfClusters);
        counts: the refined `clusteringCount`."""
        Ws = [np.ascontiguousarray(w[1] if isinstance(w, tuple) else w, dtype=np.float64) for w in factors_W]
        if len(Ws) != len(mappings.items_in_cluster):
            raise ValueError("factors_W must hold one matrix per parent cluster")
        for c, w in enumerate(Ws):
            if w.ndim != 2 or (w.shape[0] != mappings.items_in_cluster[c] and w.size):
                raise ValueError("W of parent cluster %d must be itemsInCluster x subClusters" % c)
        m_c = _i32(mappings.items_in_cluster)
        k_c = _i32([w.shape[1] for w in Ws])
        flat = np.concatenate([w.ravel() for w in Ws]) if Ws else np.zeros(0)
        item = _i32(mappings.item)
        cnt = None if counts is None else _i32(counts)
        _check(self._lib.fy_foldin_add_level(self._h, len(Ws), m_c.ctypes.data, k_c.ctypes.data, item.ctypes.data if len(item) else None,
                                             flat.ctypes.data if len(flat) else None, int(stride),
                                             cnt.ctypes.data if cnt is not None and len(cnt) else None, len(cnt) if cnt is not None else 0))
        return self

    def assign(self, profiles, iterations=10, first_iteration=1, h0=None, rank=0, world=1):
        """profiles: the two forms ``recommend_profiles`` takes.  h0: (profiles x k) starting rows of ALL profiles given (top level);
        None = uniform 1 / k.  Returns a ``FoldInAssignment`` for this rank's range of the list."""
        q, keep = _itemcf_profiles(profiles, "whole", 0.0)
        if h0 is not None:
            h0 = np.ascontiguousarray(h0, dtype=np.float64)
            if h0.shape != (q.n_profiles, self.k):
                raise ValueError("h0 must be profiles x k")
        out = C.c_void_p()
        _check(self._lib.fy_foldin_assign(self._h, C.byref(q), int(iterations), int(first_iteration),
                                          h0.ctypes.data if h0 is not None and h0.size else None, int(rank), int(world), C.byref(out)))
        del keep
        return FoldInAssignment(out, self.k, self._ctx)

    def close(self):
        if getattr(self, "_h", None):
            if self._ctx._h:      # the model's HBM goes with its context
                self._lib.fy_foldin_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RMRecommenderDriver:
    """The reference's production entry point in one call (M/rmrecommender/RMRecommenderDriver.java:164-206):

      numberOfIterations > 0      PPC factorisation -> cluster assignment -> cluster refinement if usersPerSubCluster > 0 -> counts
      numberOfIterations <= 0     the caller's ``clustering`` (and ``clustering_count``) are used
      numberOfRecommendations > 0 the RM2 job runs on the result

    Configuration keys: numberOfUsers, numberOfItems, numberOfClusters (required, :90-92) and the driver's own defaults
    (:93-119) for usersPerSubCluster (-1), numberOfIterations (10), numberOfRecommendations (1000), normalizationFrequency (12),
    lambda, filterUsers, and smoothing / mu / delta, which reach the RM2 stage as they are (``RM2Job``).  One ``Ratings`` object
    serves every stage.  ``run`` returns ``(recommendations, (users, clusters,
    counts))``: the ``Recommendations`` of ``RM2Job.run`` (None when numberOfRecommendations <= 0) and the clustering the RM2 job
    was -- or would have been -- given.  After refinement the cluster ids are parent * ceil(numberOfUsers / numberOfClusters) +
    sub-cluster, sparse in a long ``counts``; the RM2 job then runs with numberOfClusters = len(counts) (the reference sets the
    NUMBER of sub-clusters there, :262, which its own ids exceed)."""

    DEFAULTS = {"usersPerSubCluster": -1, "numberOfIterations": 10, "numberOfRecommendations": 1000, "normalizationFrequency": 12}

    def __init__(self, conf, ctx=None):
        self.conf = conf
        self.ctx = ctx
        self.stats = {}
        self.fold_in = None

    def _stage_conf(self, **over):
        c = Configuration(self.conf)
        for k, v in self.DEFAULTS.items():
            if k not in c:
                c.setInt(k, v)
        for k, v in over.items():
            c.setInt(k, v)
        return c

    def run(self, ratings, H=None, W=None, clustering=None, clustering_count=None, seed=0, keep_model=False):
        """H / W: the initial matrices of the top-level PPC run (numberOfUsers x numberOfClusters, numberOfItems x
        numberOfClusters); None = uniform in (0, 1] from ``seed`` (the reference draws unpinned random matrices).  ``seed`` also
        seeds the sub-runs' matrices.  ``keep_model=True`` (numberOfIterations > 0 only) leaves ``self.fold_in``, a ``FoldIn`` over
        the run's final W and ``counts`` -- after refinement also over the parents' item lists and W_c: the mapping job then runs
        once more for the item lists, and the refinement keeps its factors.  The default changes nothing the driver does."""
        conf = self._stage_conf()
        n_users, n_items, K = (conf.getInt(k, -1) for k in ("numberOfUsers", "numberOfItems", "numberOfClusters"))
        if min(n_users, n_items, K) <= 0:
            raise ValueError("numberOfUsers, numberOfItems and numberOfClusters are required")
        iterations = conf.getInt("numberOfIterations", 10)
        if iterations <= 0 and clustering is None:
            raise ValueError("numberOfIterations <= 0 needs the caller's clustering")
        ctx = self.ctx or Context(0)
        self.ctx = ctx
        own = not isinstance(ratings, Ratings)
        r = Ratings(ctx, *ratings) if own else ratings
        self.stats = {}
        try:
            if iterations > 0:
                rng = np.random.default_rng(seed)
                H = 1.0 - rng.random((n_users, K)) if H is None else H
                W = 1.0 - rng.random((n_items, K)) if W is None else W
                ppc = NMFDriver(conf, ctx, ppc=True)
                H, W = ppc.run(r, H, W)
                self.stats["ppc"] = ppc.stats
                users, clusters, counts = ClusterAssignmentJob(ctx).run(H, first_user=1)
                refined = conf.getInt("usersPerSubCluster", -1) > 0
                if refined:
                    parents = (users, clusters)
                    refine = ClusterRefinementJob(conf, ctx, ppc=True)
                    users, clusters, counts = refine.run(r, parents, seed=seed, keep_factors=bool(keep_model))
                    self.stats["refine"] = refine.stats
                if keep_model:
                    f = conf.getInt("normalizationFrequency", -1)
                    self.fold_in = FoldIn(ctx, W, ppc=True, normalizationFrequency=f, counts=None if refined else counts)
                    if refined:
                        self.fold_in.add_level(SubClusterMappingJob(conf, ctx).run(r, parents), refine.factors, -(-n_users // K), counts=counts)
            else:
                users, clusters = _clustering_arrays(clustering)
                counts = None if clustering_count is None else _i32(clustering_count)
            rec = None
            if conf.getInt("numberOfRecommendations", 1000) > 0:
                n_ids = len(counts) if counts is not None else K
                rec = RM2Job(self._stage_conf(numberOfClusters=n_ids), ctx).run(r, clustering=(users, clusters), clustering_count=counts)
                self.stats["rm2"] = rec.stats
            return rec, (users, clusters, counts)
        finally:
            if own:
                r.close()
