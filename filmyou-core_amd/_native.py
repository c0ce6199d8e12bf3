"""ctypes declarations of include/filmyou.h and the in-tree build of libfilmyou_hip.so.

There is no CPU fallback: if the shared library is missing or does not load, importing callers get a loud
ImportError/OSError; if no gfx950 device is present, fy_context_create returns FY_ERR_NO_DEVICE.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libfilmyou_hip.so")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include", "filmyou.h")
SOURCES = ["fy_api.hip", "fy_prep.hip", "fy_rm2.hip", "fy_rm2_request.hip", "fy_rm2_profiles.hip", "fy_rm1.hip", "fy_ratings_update.hip", "fy_itemsim.hip", "fy_itemsim_request.hip", "fy_itemcf.hip", "fy_itemcf_request.hip", "fy_itemcf_profiles.hip", "fy_itemcf_pairs.hip", "fy_itemcf_estimate.hip", "fy_itemcf_because.hip", "fy_eval.hip", "fy_cluster.hip", "fy_nmf.hip", "fy_foldin.hip", "fy_refine.hip", "fy_rccl.hip", "fy_seqfile.cpp"]
HEADERS = ["fy_common.hpp", "fy_tuning.hpp", "fy_rm2_plan.hpp", "fy_rm2_tables.hpp", "fy_partition.hpp", "fy_prep.hpp", "fy_cooc.hpp", "fy_cooc_tables.hpp", "fy_rm2.hpp", "fy_rm2_kernels.hpp", "fy_rm2_launch.hpp", "fy_rm2_coop.hpp", "fy_rm2_request.hpp", "fy_rm2_profiles.hpp", "fy_rm1.hpp", "fy_ratings_update.hpp", "fy_refine.hpp", "fy_nmf_kernels.hpp", "fy_foldin.hpp", "fy_itemsim_plan.hpp", "fy_itemsim_kernels.hpp", "fy_itemsim_request.hpp", "fy_itemcf_request.hpp", "fy_itemcf_profiles.hpp", "fy_itemcf_pairs.hpp", "fy_eval.hpp"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-munsafe-fp-atomics", "-Wall",
               "-Wno-unused-result", "-ldl"]

# every symbol include/filmyou.h declares (tests check the library exports exactly these)
SYMBOLS = [
    "fy_abi_version", "fy_last_error", "fy_context_create", "fy_context_destroy", "fy_context_synchronize", "fy_context_reload_tuning", "fy_context_inject_alloc_failure",
    "fy_context_stream", "fy_ratings_create", "fy_ratings_destroy", "fy_ratings_nnz", "fy_ratings_drop_cache", "fy_ratings_apply", "fy_ratings_copy_out", "fy_rm2_prepare",
    "fy_rm2_partial_stats", "fy_rm2_stats_layout", "fy_rm2_set_global_stats", "fy_rm2_set_collectives", "fy_rccl_unique_id", "fy_rccl_create", "fy_rccl_collectives", "fy_rccl_counters", "fy_rccl_destroy", "fy_rccl_detach_context", "fy_rm2_score", "fy_rm2_score_users", "fy_result_request_stats", "fy_rm2_job_destroy", "fy_rm2_run",
    "fy_itemsim_build", "fy_itemsim_run", "fy_itemsim_prepare", "fy_itemsim_job_destroy", "fy_itemsim_rows", "fy_result_itemsim_request_stats", "fy_itemcf_recommend", "fy_itemcf_recommend_filtered", "fy_itemcf_recommend_prepared", "fy_result_itemcf_request_stats", "fy_itemsim_job_drop_rows", "fy_ratings_shifted", "fy_itemsim_pairs",
    "fy_simpairs_write_text", "fy_idfile_read", "fy_cluster_assign", "fy_nmf_factorize", "fy_result_size", "fy_result_key0", "fy_result_key1", "fy_result_value",
    "fy_result_aux", "fy_result_n_users", "fy_result_user_id", "fy_result_user_sum", "fy_result_n_items",
    "fy_result_item_id", "fy_result_item_coll", "fy_result_total_sum", "fy_result_free", "fy_result_stats",
    "fy_seqfile_read_int_int", "fy_seqfile_read_int_double", "fy_seqfile_read_intpair_float", "fy_seqfile_write_int_int",
    "fy_seqfile_write_int_double", "fy_seqfile_write_intpair_float", "fy_mapfile_write_int_double", "fy_buffer_free",
    "fy_submap_create", "fy_submap_n_users", "fy_submap_n_items", "fy_submap_nnz", "fy_submap_counts", "fy_submap_users",
    "fy_submap_items", "fy_submap_matrix", "fy_submap_destroy", "fy_cluster_refine", "fy_refined_n_users", "fy_refined_n_counts",
    "fy_refined_clustering", "fy_refined_layout", "fy_refined_h_size", "fy_refined_w_size", "fy_refined_factors",
    "fy_refined_stats", "fy_refined_free",
    "fy_ratings_holdout", "fy_result_create_lists", "fy_eval_prepare", "fy_eval_lists", "fy_eval_destroy",
    "fy_itemcf_estimate_prepared", "fy_itemcf_estimate_ratings", "fy_result_itemcf_estimate_stats", "fy_eval_estimates",
    "fy_itemcf_because_prepared", "fy_result_because_view", "fy_result_itemcf_because_stats",
    "fy_itemcf_recommend_profiles", "fy_result_itemcf_profile_stats",
    "fy_rm2_score_profiles", "fy_result_rm2_profile_stats",
    "fy_foldin_create", "fy_foldin_add_level", "fy_foldin_assign", "fy_foldin_result_n", "fy_foldin_result_assignment",
    "fy_foldin_result_factors", "fy_foldin_result_sub_size", "fy_foldin_result_sub_factors", "fy_foldin_result_stats",
    "fy_foldin_result_free", "fy_foldin_destroy",
]


def _stale():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [INCLUDE]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    """hipcc cross-compiles for gfx950 without a GPU: one object per source (in parallel, only the stale ones), then one link.
    Returns the .so path."""
    if not force and not _stale():
        build_host_driver()
        return LIB_PATH
    from concurrent.futures import ThreadPoolExecutor
    obj_dir = os.path.join(LIB_DIR, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    cflags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-ldl")]
    common = max(os.path.getmtime(d) for d in [os.path.join(CSRC, h) for h in HEADERS] + [INCLUDE])
    # objects are only as good as the command that made them: another compiler or other flags (HIPCC, HIPCC_FLAGS edited) rebuild
    # everything -- staleness by mtime alone would link objects of mixed flags
    import hashlib
    stamp_path = os.path.join(obj_dir, "flags.stamp")
    stamp = hashlib.sha256(("\0".join([os.path.realpath(hipcc)] + cflags)).encode()).hexdigest()
    try:
        with open(stamp_path) as f:
            same_flags = f.read().strip() == stamp
    except OSError:
        same_flags = False
    if not same_flags:
        force = True

    def compile_one(src):
        path, obj = os.path.join(CSRC, src), os.path.join(obj_dir, src + ".o")
        if not force and os.path.exists(obj) and os.path.getmtime(obj) > max(common, os.path.getmtime(path)):
            return obj
        cmd = [hipcc] + cflags + ["-c", "-o", obj, path]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        return obj

    with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    with open(stamp_path, "w") as f:
        f.write(stamp + "\n")
    cmd = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", LIB_PATH] + objs + ["-ldl"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    build_host_driver()
    return LIB_PATH


HOST_DIR = os.path.join(_HERE, "host")
HOST_DRIVER = os.path.join(HOST_DIR, "rm2_main")


def build_host_driver():
    """g++ build of the C++ host-side mirror's driver (filmyou-core_amd/host/rm2_main.cpp) against the library."""
    src = os.path.join(HOST_DIR, "rm2_main.cpp")
    hdr = os.path.join(HOST_DIR, "filmyou_job.hpp")
    if os.path.exists(HOST_DRIVER) and all(os.path.getmtime(HOST_DRIVER) >= os.path.getmtime(p) for p in (src, hdr, LIB_PATH)):
        return HOST_DRIVER
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", HOST_DRIVER, src, "-L" + LIB_DIR, "-lfilmyou_hip",
                    "-Wl,-rpath,$ORIGIN/../lib"], check=True)
    return HOST_DRIVER


class RM2Params(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("number_of_items", C.c_int32), ("number_of_recommendations", C.c_int32),
                ("filter_users", C.c_int32), ("number_of_clusters", C.c_int32), ("rank", C.c_int32),
                ("world", C.c_int32), ("flags", C.c_uint32), ("workspace_bytes", C.c_int64)]


# fy_collectives: RCCL-shaped callbacks (device pointers, hipStream_t), see include/filmyou.h
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
REDUCE_SCATTER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)


class Collectives(C.Structure):
    _fields_ = [("user", C.c_void_p), ("all_gather", ALL_GATHER_FN), ("reduce_scatter_f32", REDUCE_SCATTER_FN)]


class NMFParams(C.Structure):
    _fields_ = [("number_of_users", C.c_int32), ("number_of_items", C.c_int32), ("number_of_clusters", C.c_int32),
                ("number_of_iterations", C.c_int32), ("ppc", C.c_int32), ("normalization_frequency", C.c_int32)]


class RefineParams(C.Structure):
    _fields_ = [("number_of_users", C.c_int32), ("number_of_clusters", C.c_int32), ("users_per_sub_cluster", C.c_int32),
                ("number_of_iterations", C.c_int32), ("ppc", C.c_int32), ("normalization_frequency", C.c_int32),
                ("seed", C.c_uint64)]


class RefineStats(C.Structure):
    _fields_ = [("ms_mappings", C.c_double), ("ms_iterations", C.c_double), ("ms_assign", C.c_double), ("ms_total", C.c_double),
                ("launches", C.c_int64), ("sum_users", C.c_int64), ("sum_items", C.c_int64), ("sum_k", C.c_int64),
                ("nnz", C.c_int64), ("collisions", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ItemSimParams(C.Structure):
    _fields_ = [("similarity", C.c_int32), ("max_similarities_per_item", C.c_int32), ("exclude_self", C.c_int32),
                ("has_threshold", C.c_int32), ("threshold", C.c_double), ("rank", C.c_int32), ("world", C.c_int32),
                ("flags", C.c_uint32), ("min_prefs_per_user", C.c_int32), ("max_prefs_per_user", C.c_int32)]


class ItemCFParams(C.Structure):
    _fields_ = [("num_recommendations", C.c_int32), ("max_prefs_per_user", C.c_int32), ("boolean_data", C.c_int32),
                ("rank", C.c_int32), ("world", C.c_int32), ("flags", C.c_uint32)]


class ItemCFFilter(C.Structure):
    _fields_ = [("has_users", C.c_int32), ("has_items", C.c_int32), ("n_users", C.c_int64), ("users", C.c_void_p),
                ("n_items", C.c_int64), ("items", C.c_void_p)]


class RM2Request(C.Structure):
    _fields_ = [("n_users", C.c_int64), ("users", C.c_void_p)]


class RM2RequestStats(C.Structure):
    _fields_ = [("users_asked", C.c_int64), ("users_known", C.c_int64), ("clusters_touched", C.c_int64), ("batches", C.c_int64),
                ("slab_rows", C.c_int64), ("slab_bytes_peak", C.c_int64), ("slab_pair_contribs", C.c_int64),
                ("full_pass_clusters", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ItemSimRequest(C.Structure):
    _fields_ = [("n_items", C.c_int64), ("items", C.c_void_p)]


class ItemSimRequestStats(C.Structure):
    _fields_ = [("items_asked", C.c_int64), ("items_known", C.c_int64), ("rows_emitted", C.c_int64), ("batches", C.c_int64),
                ("pair_contribs", C.c_int64), ("chunks", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ItemCFRequestStats(C.Structure):
    _fields_ = [("users_asked", C.c_int64), ("users_known", C.c_int64), ("items_needed", C.c_int64), ("rows_built", C.c_int64),
                ("rows_from_store", C.c_int64), ("rows_stored", C.c_int64), ("pair_contribs", C.c_int64), ("batches", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


FY_PROFILE_WHOLE, FY_PROFILE_ON_RESIDENT = 0, 1


class ItemCFProfiles(C.Structure):
    _fields_ = [("n_profiles", C.c_int64), ("user", C.c_void_p), ("start", C.c_void_p), ("item", C.c_void_p), ("score", C.c_void_p),
                ("remove", C.c_void_p), ("base", C.c_int32)]


class ItemCFProfileStats(C.Structure):
    _fields_ = [("profiles_asked", C.c_int64), ("profiles_mine", C.c_int64), ("profiles_scored", C.c_int64), ("profiles_empty", C.c_int64),
                ("users_unknown", C.c_int64), ("entries", C.c_int64), ("entries_unknown_item", C.c_int64), ("entries_superseded", C.c_int64),
                ("removes_hit", C.c_int64), ("removes_missed", C.c_int64), ("prefs_composed", C.c_int64), ("items_needed", C.c_int64),
                ("rows_built", C.c_int64), ("rows_from_store", C.c_int64), ("rows_stored", C.c_int64), ("pair_contribs", C.c_int64),
                ("batches", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RM2Profiles(C.Structure):
    _fields_ = [("n_profiles", C.c_int64), ("user", C.c_void_p), ("start", C.c_void_p), ("item", C.c_void_p), ("score", C.c_void_p),
                ("remove", C.c_void_p), ("cluster", C.c_void_p), ("base", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32)]


class RM2ProfileStats(C.Structure):
    _fields_ = [("profiles_asked", C.c_int64), ("profiles_mine", C.c_int64), ("profiles_scored", C.c_int64), ("profiles_empty", C.c_int64),
                ("users_unknown", C.c_int64), ("users_filtered", C.c_int64), ("entries", C.c_int64), ("entries_unknown_item", C.c_int64),
                ("entries_nonpositive", C.c_int64), ("entries_superseded", C.c_int64), ("removes_hit", C.c_int64),
                ("removes_missed", C.c_int64), ("items_composed", C.c_int64), ("clusters_touched", C.c_int64), ("batches", C.c_int64),
                ("slab_rows", C.c_int64), ("slab_bytes_peak", C.c_int64), ("slab_pair_contribs", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


FY_FOLDIN_OK, FY_FOLDIN_EMPTY, FY_FOLDIN_NO_CLUSTER, FY_FOLDIN_EMPTY_IN_PARENT = 0, 1, 2, 3


class FoldInParams(C.Structure):
    _fields_ = [("number_of_items", C.c_int32), ("number_of_clusters", C.c_int32), ("ppc", C.c_int32),
                ("normalization_frequency", C.c_int32)]


class FoldInStats(C.Structure):
    _fields_ = [("profiles_asked", C.c_int64), ("profiles_mine", C.c_int64), ("profiles_assigned", C.c_int64), ("profiles_empty", C.c_int64),
                ("profiles_no_cluster", C.c_int64), ("profiles_empty_in_parent", C.c_int64), ("entries", C.c_int64),
                ("entries_out_of_range", C.c_int64), ("entries_superseded", C.c_int64), ("entries_removed", C.c_int64),
                ("entries_nonpositive", C.c_int64), ("items_composed", C.c_int64), ("items_in_parent", C.c_int64), ("collisions", C.c_int64),
                ("launches", C.c_int64), ("ms_ingest", C.c_double), ("ms_level1", C.c_double), ("ms_level2", C.c_double),
                ("ms_total", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RatingsUpdateStats(C.Structure):
    _fields_ = [("n_writes", C.c_int64), ("n_superseded", C.c_int64), ("n_replaced", C.c_int64), ("n_inserted", C.c_int64),
                ("n_deleted", C.c_int64), ("n_delete_missed", C.c_int64), ("n_source_dropped", C.c_int64), ("nnz_out", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class EvalParams(C.Structure):
    _fields_ = [("n_cutoffs", C.c_int32), ("cutoffs", C.c_int32 * 8), ("gain", C.c_int32), ("flags", C.c_uint32),
                ("relevance_threshold", C.c_double)]


class EvalSums(C.Structure):
    _fields_ = [("lists", C.c_int64), ("users_evaluated", C.c_int64), ("lists_without_relevant", C.c_int64),
                ("relevant_users", C.c_int64), ("relevant_entries", C.c_int64), ("distinct_items", C.c_int64),
                ("n_cutoffs", C.c_int32), ("reserved", C.c_int32), ("cutoffs", C.c_int32 * 8), ("hits", C.c_int64 * 8),
                ("users_hit", C.c_int64 * 8), ("recall", C.c_double * 8), ("ap", C.c_double * 8), ("rr", C.c_double * 8),
                ("ndcg", C.c_double * 8), ("ms", C.c_double)]


class ItemCFPairs(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("users", C.c_void_p), ("items", C.c_void_p), ("location", C.c_int)]


class ItemCFEstimateStats(C.Structure):
    _fields_ = [("pairs_asked", C.c_int64), ("pair_offset", C.c_int64), ("by_status", C.c_int64 * 8), ("users_known", C.c_int64),
                ("targets", C.c_int64), ("chunks", C.c_int64), ("items_needed", C.c_int64), ("rows_built", C.c_int64),
                ("rows_from_store", C.c_int64), ("rows_stored", C.c_int64), ("pair_contribs", C.c_int64), ("batches", C.c_int64),
                ("row_entries_walked", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["by_status"] = list(self.by_status)
        return d


FY_BECAUSE_MAX = 64


class ItemCFBecauseView(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("start", C.c_void_p), ("user", C.c_void_p), ("item", C.c_void_p), ("estimate", C.c_void_p),
                ("status", C.c_void_p), ("contributors", C.c_void_p), ("pref", C.c_void_p)]


class ItemCFBecauseStats(C.Structure):
    _fields_ = [("pairs_asked", C.c_int64), ("pair_offset", C.c_int64), ("by_status", C.c_int64 * 8), ("users_known", C.c_int64),
                ("targets", C.c_int64), ("rows", C.c_int64), ("contributors", C.c_int64), ("items_needed", C.c_int64),
                ("rows_built", C.c_int64), ("rows_from_store", C.c_int64), ("rows_stored", C.c_int64), ("pair_contribs", C.c_int64),
                ("batches", C.c_int64), ("row_entries_walked", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["by_status"] = list(self.by_status)
        return d


class EvalErrorParams(C.Structure):
    _fields_ = [("has_clamp", C.c_int32), ("reserved", C.c_int32), ("clamp_lo", C.c_double), ("clamp_hi", C.c_double)]


class EvalErrors(C.Structure):
    _fields_ = [("pairs", C.c_int64), ("estimated", C.c_int64), ("truth_not_finite", C.c_int64), ("by_status", C.c_int64 * 8),
                ("sum_abs", C.c_double), ("sum_sq", C.c_double), ("sum_err", C.c_double), ("ms", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("nnz", C.c_int64), ("n_users", C.c_int64), ("n_items", C.c_int64),
                ("n_clusters_nonempty", C.c_int64), ("users_scored", C.c_int64), ("recs", C.c_int64),
                ("log_terms", C.c_int64), ("pair_contribs", C.c_int64), ("unordered_pairs", C.c_int64),
                ("ms_prepare", C.c_double), ("ms_cooc", C.c_double), ("ms_score", C.c_double),
                ("ms_topn", C.c_double), ("ms_total", C.c_double), ("score_launches", C.c_int64),
                ("cooc_launches", C.c_int64), ("blocks_total", C.c_int64), ("blocks_survived", C.c_int64),
                ("log_terms_evaluated", C.c_int64), ("prune_fallbacks", C.c_int64), ("ms_tables", C.c_double), ("ms_mirror", C.c_double), ("topn_select_users", C.c_int64),
                ("panel_clusters", C.c_int64), ("stray_blocks", C.c_int64), ("bound_repairs", C.c_int64),
                ("isim_candidates", C.c_int64), ("isim_redone_rows", C.c_int64),
                ("prepared_from_cache", C.c_int64), ("tables_from_cache", C.c_int64),
                ("cooc_segments", C.c_int64), ("cooc_matrix_bytes", C.c_int64), ("rows_refined", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def load():
    """dlopen the in-tree library and declare argument types.  Raises OSError when it is missing (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(the HIP extension is required; there is no CPU fallback)" % LIB_PATH)
    # One HIP runtime per process: the torch wheel bundles its own libamdhip64.so / libhsa-runtime64.so under the same
    # SONAMEs as /opt/rocm's.  Whichever is loaded first serves both torch and this library; if this library came first,
    # torch would later run on a runtime it was not built with (observed: "No HIP GPUs are available" from torch.cuda.init()).
    # The Python host layer hands torch tensors / streams to the library anyway, so torch goes first.  A host without torch
    # (the JNI shim, the C++ driver) simply uses the system ROCm.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i64, i32, pvp = C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)
    L.fy_abi_version.restype = C.c_int
    L.fy_last_error.restype = C.c_char_p
    L.fy_context_create.argtypes = [C.c_int, pvp]
    L.fy_context_destroy.argtypes = [vp]
    L.fy_context_destroy.restype = None
    L.fy_context_synchronize.argtypes = [vp]
    L.fy_context_inject_alloc_failure.argtypes = [vp, i64]
    L.fy_context_reload_tuning.argtypes = [vp]
    L.fy_context_stream.argtypes = [vp]
    L.fy_context_stream.restype = vp
    L.fy_ratings_create.argtypes = [vp, i64, vp, vp, vp, C.c_int, pvp]
    L.fy_ratings_destroy.argtypes = [vp]
    L.fy_ratings_destroy.restype = None
    L.fy_ratings_nnz.argtypes = [vp]
    L.fy_ratings_nnz.restype = i64
    L.fy_ratings_drop_cache.argtypes = [vp]
    L.fy_ratings_drop_cache.restype = None
    L.fy_ratings_apply.argtypes = [vp, vp, i64, vp, vp, vp, vp, C.c_int, pvp, C.POINTER(RatingsUpdateStats)]
    L.fy_ratings_copy_out.argtypes = [vp, vp, vp, vp]
    L.fy_rm2_prepare.argtypes = [vp, C.POINTER(RM2Params), vp, i64, vp, vp, vp, pvp]
    L.fy_rm2_partial_stats.argtypes = [vp, pvp, C.POINTER(i64)]
    L.fy_rm2_set_global_stats.argtypes = [vp, vp, i32]
    L.fy_rm2_stats_layout.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.fy_nmf_factorize.argtypes = [vp, C.POINTER(NMFParams), vp, vp, vp, C.POINTER(Stats)]
    L.fy_cluster_assign.argtypes = [vp, i32, i32, vp, C.c_int, i32, i32, i32, vp, vp, vp]
    L.fy_rm2_set_collectives.argtypes = [vp, C.POINTER(Collectives)]
    L.fy_rccl_unique_id.argtypes = [vp]
    L.fy_rccl_create.argtypes = [vp, C.c_int, C.c_int, vp, pvp]
    L.fy_rccl_collectives.argtypes = [vp, C.POINTER(Collectives)]
    L.fy_rccl_counters.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.fy_rccl_destroy.argtypes = [vp]
    L.fy_rccl_destroy.restype = None
    L.fy_rccl_detach_context.argtypes = [vp]
    L.fy_rccl_detach_context.restype = None
    L.fy_rm2_score.argtypes = [vp, pvp]
    L.fy_rm2_score_users.argtypes = [vp, C.POINTER(RM2Request), pvp]
    L.fy_result_request_stats.argtypes = [vp, C.POINTER(RM2RequestStats)]
    L.fy_rm2_job_destroy.argtypes = [vp]
    L.fy_rm2_job_destroy.restype = None
    L.fy_rm2_run.argtypes = [C.POINTER(RM2Params), i64, vp, vp, vp, i64, vp, vp, vp, pvp]
    L.fy_itemsim_build.argtypes = [vp, C.POINTER(ItemSimParams), vp, pvp]
    L.fy_itemsim_run.argtypes = [C.POINTER(ItemSimParams), i64, vp, vp, vp, pvp]
    L.fy_itemsim_prepare.argtypes = [vp, C.POINTER(ItemSimParams), vp, pvp]
    L.fy_itemsim_job_destroy.argtypes = [vp]
    L.fy_itemsim_job_destroy.restype = None
    L.fy_itemsim_rows.argtypes = [vp, C.POINTER(ItemSimRequest), pvp]
    L.fy_result_itemsim_request_stats.argtypes = [vp, C.POINTER(ItemSimRequestStats)]
    L.fy_itemcf_recommend.argtypes = [vp, C.POINTER(ItemCFParams), vp, vp, pvp]
    L.fy_itemcf_recommend_filtered.argtypes = [vp, C.POINTER(ItemCFParams), C.POINTER(ItemCFFilter), vp, vp, pvp]
    L.fy_itemcf_recommend_prepared.argtypes = [vp, C.POINTER(ItemCFParams), C.POINTER(ItemCFFilter), pvp]
    L.fy_result_itemcf_request_stats.argtypes = [vp, C.POINTER(ItemCFRequestStats)]
    L.fy_itemsim_job_drop_rows.argtypes = [vp]
    L.fy_itemsim_job_drop_rows.restype = None
    L.fy_ratings_shifted.argtypes = [vp, vp, C.c_float, pvp]
    L.fy_itemsim_pairs.argtypes = [vp, vp, pvp]
    for name, rt in (("size", i64), ("key0", vp), ("key1", vp), ("value", vp), ("aux", vp), ("n_users", i64),
                     ("user_id", vp), ("user_sum", vp), ("n_items", i64), ("item_id", vp), ("item_coll", vp),
                     ("total_sum", C.c_double)):
        f = getattr(L, "fy_result_" + name)
        f.argtypes = [vp]
        f.restype = rt
    L.fy_result_free.argtypes = [vp]
    L.fy_result_free.restype = None
    L.fy_result_stats.argtypes = [vp, C.POINTER(Stats)]
    cp, pi64 = C.c_char_p, C.POINTER(i64)
    L.fy_seqfile_read_int_int.argtypes = [cp, pi64, pvp, pvp]
    L.fy_seqfile_read_int_double.argtypes = [cp, pi64, pvp, pvp]
    L.fy_seqfile_read_intpair_float.argtypes = [cp, pi64, pvp, pvp, pvp]
    L.fy_seqfile_write_int_int.argtypes = [cp, i64, vp, vp]
    L.fy_seqfile_write_int_double.argtypes = [cp, i64, vp, vp]
    L.fy_seqfile_write_intpair_float.argtypes = [cp, i64, vp, vp, vp]
    L.fy_mapfile_write_int_double.argtypes = [cp, i64, vp, vp]
    L.fy_simpairs_write_text.argtypes = [cp, i64, vp, vp, vp]
    L.fy_idfile_read.argtypes = [cp, pi64, pvp]
    L.fy_buffer_free.argtypes = [vp]
    L.fy_buffer_free.restype = None
    L.fy_submap_create.argtypes = [vp, vp, i32, i64, vp, vp, pvp]
    for name in ("fy_submap_n_users", "fy_submap_n_items", "fy_submap_nnz", "fy_refined_n_users", "fy_refined_n_counts",
                 "fy_refined_h_size", "fy_refined_w_size"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = i64
    L.fy_submap_counts.argtypes = [vp, vp, vp]
    L.fy_submap_users.argtypes = [vp, vp, vp, vp]
    L.fy_submap_items.argtypes = [vp, vp, vp, vp]
    L.fy_submap_matrix.argtypes = [vp, C.c_int, vp, vp, vp]
    L.fy_submap_destroy.argtypes = [vp]
    L.fy_submap_destroy.restype = None
    L.fy_cluster_refine.argtypes = [vp, C.POINTER(RefineParams), vp, i64, vp, vp, vp, vp, pvp]
    L.fy_refined_clustering.argtypes = [vp, vp, vp, vp]
    L.fy_refined_layout.argtypes = [vp, vp, vp, vp]
    L.fy_refined_factors.argtypes = [vp, vp, vp]
    L.fy_refined_stats.argtypes = [vp, C.POINTER(RefineStats)]
    L.fy_refined_free.argtypes = [vp]
    L.fy_refined_free.restype = None
    L.fy_ratings_holdout.argtypes = [vp, vp, C.c_double, C.c_uint64, pvp, pvp]
    L.fy_result_create_lists.argtypes = [vp, i64, vp, vp, vp, C.c_int, pvp]
    L.fy_eval_prepare.argtypes = [vp, C.POINTER(EvalParams), vp, pvp]
    L.fy_eval_lists.argtypes = [vp, vp, C.POINTER(EvalSums), vp, vp]
    L.fy_eval_destroy.argtypes = [vp]
    L.fy_eval_destroy.restype = None
    L.fy_itemcf_estimate_prepared.argtypes = [vp, C.POINTER(ItemCFParams), C.POINTER(ItemCFPairs), pvp]
    L.fy_itemcf_estimate_ratings.argtypes = [vp, C.POINTER(ItemCFParams), vp, pvp]
    L.fy_result_itemcf_estimate_stats.argtypes = [vp, C.POINTER(ItemCFEstimateStats)]
    L.fy_eval_estimates.argtypes = [vp, vp, vp, C.POINTER(EvalErrorParams), C.POINTER(EvalErrors)]
    L.fy_itemcf_because_prepared.argtypes = [vp, C.POINTER(ItemCFParams), C.POINTER(ItemCFPairs), i32, pvp]
    L.fy_result_because_view.argtypes = [vp, C.POINTER(ItemCFBecauseView)]
    L.fy_result_itemcf_because_stats.argtypes = [vp, C.POINTER(ItemCFBecauseStats)]
    L.fy_itemcf_recommend_profiles.argtypes = [vp, C.POINTER(ItemCFParams), C.POINTER(ItemCFProfiles), C.POINTER(ItemCFFilter), pvp]
    L.fy_result_itemcf_profile_stats.argtypes = [vp, C.POINTER(ItemCFProfileStats)]
    L.fy_rm2_score_profiles.argtypes = [vp, C.POINTER(RM2Profiles), pvp]
    L.fy_result_rm2_profile_stats.argtypes = [vp, C.POINTER(RM2ProfileStats)]
    L.fy_foldin_create.argtypes = [vp, C.POINTER(FoldInParams), vp, C.c_int, vp, i64, pvp]
    L.fy_foldin_add_level.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, i64]
    L.fy_foldin_assign.argtypes = [vp, C.POINTER(ItemCFProfiles), i32, i32, vp, i32, i32, pvp]
    for name in ("fy_foldin_result_n", "fy_foldin_result_sub_size"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = i64
    L.fy_foldin_result_assignment.argtypes = [vp, vp, vp, vp, vp]
    L.fy_foldin_result_factors.argtypes = [vp, vp]
    L.fy_foldin_result_sub_factors.argtypes = [vp, vp, vp]
    L.fy_foldin_result_stats.argtypes = [vp, C.POINTER(FoldInStats)]
    L.fy_foldin_result_free.argtypes = [vp]
    L.fy_foldin_result_free.restype = None
    L.fy_foldin_destroy.argtypes = [vp]
    L.fy_foldin_destroy.restype = None
    _lib = L
    return L
