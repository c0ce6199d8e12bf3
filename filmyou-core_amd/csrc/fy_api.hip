// fy_api.hip -- the extern "C" surface declared in include/filmyou.h: context, ratings, results, error plumbing.
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <new>
#include <unordered_map>

#include "fy_prep.hpp"
#include "fy_rm2.hpp"
#include "fy_ratings_update.hpp"
#include "fy_rm2_request.hpp"
#include "fy_rm2_profiles.hpp"
#include "fy_itemsim_request.hpp"
#include "fy_itemcf_request.hpp"
#include "fy_itemcf_profiles.hpp"
#include "fy_eval.hpp"
#include "fy_foldin.hpp"

namespace fy {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
const char* last_error() { return g_err; }
}  // namespace fy

using namespace fy;

// the ONE place the library reads its environment (fy_context_create, fy_context_reload_tuning)
void fy::load_tuning_from_env(Tuning& t) {
    t = Tuning{};
    if (const char* e = getenv("FY_M24")) t.pack24 = atoi(e) != 0;
    if (const char* e = getenv("FY_M24_MIN_ITEMS")) t.pack24_min_items = std::max(0, atoi(e));
    if (const char* e = getenv("FY_SCORE_SLICES")) t.max_slices = atoi(e);
    if (const char* e = getenv("FY_SCORE_UPW")) { int v = atoi(e); if (v >= 1) t.users_per_wave = v; }
    if (const char* e = getenv("FY_PRUNE")) t.prune = atoi(e) != 0;
    if (const char* e = getenv("FY_LAZY_MIRROR")) t.lazy_mirror = atoi(e) != 0;
    if (const char* e = getenv("FY_REFINE")) t.refine = atoi(e) != 0;
    if (const char* e = getenv("FY_REFINE_C")) { double v = atof(e); if (v >= 0.0 && v < 1e6) t.refine_c = (float)v; }
    if (const char* e = getenv("FY_FULL_WALK_SPARSE")) t.full_walk_sparse = atoi(e) != 0;
    if (const char* e = getenv("FY_PREP_PACKED")) t.prep_packed = atoi(e) != 0;
    if (const char* e = getenv("FY_OVERLAP_VALUES")) t.overlap_values = atoi(e) != 0;
    if (const char* e = getenv("FY_SHARD_PREP")) t.shard_prep = atoi(e) != 0;
    if (const char* e = getenv("FY_SUP_BOUNDS")) t.sup_bounds = atoi(e) != 0;
    if (const char* e = getenv("FY_COOP")) t.coop = atoi(e) != 0;
    if (const char* e = getenv("FY_COOP_FORCE")) t.coop_force = atoi(e) != 0;
    if (const char* e = getenv("FY_COOC_PK")) t.cooc_pk = atoi(e) != 0;
    if (const char* e = getenv("FY_COOC_F32")) t.cooc_f32 = atoi(e) != 0;
    if (const char* e = getenv("FY_COOC_HALF")) t.cooc_half = atoi(e) != 0;
    if (const char* e = getenv("FY_COOC_RECT")) t.cooc_rect = atoi(e) != 0;
    if (const char* e = getenv("FY_COOC_FX")) t.cooc_fx = atoi(e) != 0;
    if (const char* e = getenv("FY_PANEL_MIN_CLUSTERS")) { int v = atoi(e); if (v >= 1) t.panel_min_clusters = v; }
    if (const char* e = getenv("FY_PANEL_COLS")) { int v = atoi(e); if (v >= 256) { t.panel_cols = v; t.panel_wide_below_users = 0; } }
    if (const char* e = getenv("FY_PANEL_WIDE_BELOW_USERS")) { int v = atoi(e); if (v >= 0) t.panel_wide_below_users = v; }
    if (const char* e = getenv("FY_PANEL_MAX_CH")) { int v = atoi(e); if (v >= 256) t.panel_max_ch = v; }
    if (const char* e = getenv("FY_COOC_PLANES")) t.cooc_planes = atoi(e) != 0;
    if (const char* e = getenv("FY_SCORE_HEAVY")) { int v = atoi(e); if (v >= 0) t.score_heavy = v; }
    if (const char* e = getenv("FY_SCORE_WALK")) t.score_walk = atoi(e) != 0;
    if (const char* e = getenv("FY_COOC_EPI")) t.cooc_epi = atoi(e) != 0;
    if (const char* e = getenv("FY_TOPN_SEED_XL")) t.topn_seed_xl = atoi(e) != 0;
    if (const char* e = getenv("FY_PANEL_REPAIR")) t.panel_repair = atoi(e) != 0;
    if (const char* e = getenv("FY_PANEL_MULTI_LAUNCH")) t.panel_multi_launch = atoi(e) != 0;
    if (const char* e = getenv("FY_FLAT")) t.flat_batch = atoi(e) != 0;
    if (const char* e = getenv("FY_PANEL_SYM")) t.panel_sym = atoi(e) != 0;
    if (const char* e = getenv("FY_DEBUG_SYNC")) t.debug_sync = atoi(e);
    if (const char* e = getenv("FY_PANEL_GROUP_MB")) t.panel_group_bytes = std::max<int64_t>(0, (int64_t)atoll(e)) << 20;      // (0 = default)
    if (const char* e = getenv("FY_FLAT_BUDGET_MB")) t.flat_budget = std::max<int64_t>(0, (int64_t)atoll(e)) << 20;
    if (const char* e = getenv("FY_PANEL_TWO_PHASE")) t.panel_two_phase = atoi(e) != 0;
    if (const char* e = getenv("FY_PANEL_LANES")) { int v = atoi(e); if (v >= 1 && v <= 8) t.panel_lanes = v; }
    if (const char* e = getenv("FY_PRUNE_MIN_ITEMS")) { t.prune_min_items = atoi(e); t.prune_min_users = 0; }   // (a forced item threshold -- tests -- lifts the user threshold too)
    if (const char* e = getenv("FY_PRUNE_MIN_USERS")) { int v = atoi(e); if (v >= 0) t.prune_min_users = v; }
    if (const char* e = getenv("FY_SEED_CHUNKS")) { int v = atoi(e); if (v >= 0 && v <= 40) { t.seed_chunks = v; t.seed_forced = v > 0; } }     // (40 = SEED_CHUNKS_MAX, fy_rm2_kernels.hpp)
    if (const char* e = getenv("FY_WORKSPACE_GB")) { long v = atol(e); if (v >= 1) t.workspace_default = (int64_t)v << 30; }
    if (const char* e = getenv("FY_LANES")) { int v = atoi(e); if (v >= 1 && v <= 8) { t.lanes = v; t.lanes_forced = true; } }
    if (const char* e = getenv("FY_COOC_BLOCK")) { int v = atoi(e); if (v == 256 || v == 512 || v == 1024) t.cooc_block = v; }
    if (const char* e = getenv("FY_COOC_MAX_CH")) { int v = atoi(e); if (v >= 64 && v <= 20224) { t.cooc_max_ch = v; t.cooc_max_ch_forced = true; } }
    if (const char* e = getenv("FY_TOPN_FORCE_SELECT")) t.force_select = atoi(e) != 0;
    if (const char* e = getenv("FY_MAX_SURV_FRAC")) { double v = atof(e); if (v >= 0.0) t.max_surv_frac = v; }
    if (const char* e = getenv("FY_REQ_FULL_SHARE")) { double v = atof(e); if (v >= 0.0) t.req_full_share = v; }
    if (const char* e = getenv("FY_REQ_CHUNK")) { int v = atoi(e); if (v >= 64 && v <= 16384 && v % 64 == 0) t.req_chunk = v; }
    if (const char* e = getenv("FY_RM1_NBR_CHUNK")) { int v = atoi(e); if (v >= 1 && v <= (1 << 20)) t.rm1_nbr_chunk = v; }
    if (const char* e = getenv("FY_RM1_COL_CHUNK")) { int v = atoi(e); if (v >= 1 && v <= (1 << 20)) t.rm1_col_chunk = v; }
    if (const char* e = getenv("FY_UPD_LDS_KEYS")) { int v = atoi(e); if (v >= 0 && v <= fy::UPD_LDS_KEYS_MAX) t.upd_lds_keys = v; }
    if (const char* e = getenv("FY_ISIM_HEAVY")) t.isim_heavy = std::max(0, atoi(e));
    if (const char* e = getenv("FY_ISIM_GRAM")) t.isim_gram = atoi(e) != 0;
    if (const char* e = getenv("FY_ISIM_GRAM_MIN_ITEMS")) t.isim_gram_min_items = std::max(0, atoi(e));
    if (const char* e = getenv("FY_ISIM_CAPG")) { int v = atoi(e); if (v >= 1 && v <= 2040) t.isim_capg = v; }
    if (const char* e = getenv("FY_ISIM_ACC32")) t.isim_acc32 = atoi(e) != 0;
    if (const char* e = getenv("FY_ISIM_PIECE")) { int v = atoi(e); if (v >= 64 && v <= 8192 && v % 64 == 0) t.isim_piece = v; }
    if (const char* e = getenv("FY_ISIM_REQ_CHUNK")) { int v = atoi(e); if (v >= 64 && v <= 16384 && v % 64 == 0) t.isim_req_chunk = v; }
    if (const char* e = getenv("FY_ISIM_REQ_ROWS")) t.isim_req_rows = std::max(0, atoi(e));
    if (const char* e = getenv("FY_ICF_EST_CHUNK")) { int v = atoi(e); if (v >= 1 && v <= fy::ICF_EST_CHUNK_MAX) t.icf_est_chunk = v; }
}

// Every entry point that reaches the GPU selects its context's device first: allocations, new streams and kernel attributes
// go to the calling thread's CURRENT device, and a host that drives several GPUs from one process (or hands a job to
// another thread) would otherwise build one context's job in another GPU's memory.  The job handle is opaque in this file,
// so the contexts of live jobs are kept here (fy_rm2_prepare ... fy_rm2_job_destroy).
namespace {
// (never destroyed: a host may release its last job from a static destructor of its own, after this library's would have run)
std::mutex& g_jobs_mu = *new std::mutex;
std::unordered_map<const fy_rm2_job*, fy::Context*>& g_jobs = *new std::unordered_map<const fy_rm2_job*, fy::Context*>;
fy::Context* job_context(const fy_rm2_job* j) {
    std::lock_guard<std::mutex> g(g_jobs_mu);
    auto it = g_jobs.find(j);
    return it == g_jobs.end() ? nullptr : it->second;
}
inline void select_device(const fy::Context* ctx) {
    if (ctx) FY_HIP(hipSetDevice(ctx->device));
}
}  // namespace

// every entry point: no exception may cross the ABI
#define FY_TRY try {
#define FY_CATCH                                                           \
    }                                                                      \
    catch (const fy::Failure& f) { return f.code; }                        \
    catch (const std::bad_alloc&) {                                        \
        fy::set_error("host allocation failed");                           \
        return FY_ERR_OUT_OF_MEMORY;                                       \
    }                                                                      \
    catch (const std::exception& e) {                                      \
        fy::set_error("unexpected: %s", e.what());                         \
        return FY_ERR_HIP;                                                 \
    }                                                                      \
    return FY_OK;

extern "C" {

int fy_abi_version(void) { return FY_ABI_VERSION; }
const char* fy_last_error(void) { return fy::last_error(); }

int fy_context_create(int device_ordinal, fy_context** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    FY_TRY
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        FY_FAIL(FY_ERR_NO_DEVICE, "no HIP device is visible (%s); this library has no CPU fallback",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    }
    if (device_ordinal < 0 || device_ordinal >= n) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "device %d of %d", device_ordinal, n);
    FY_HIP(hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    FY_HIP(hipGetDeviceProperties(&prop, device_ordinal));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        FY_FAIL(FY_ERR_NO_DEVICE, "device %d is %s; the kernels are built for gfx950 (MI355X) only", device_ordinal, prop.gcnArchName);
    std::unique_ptr<fy_context> c(new fy_context);
    c->c.device = device_ordinal;
    c->c.num_cus = prop.multiProcessorCount;
    c->c.total_mem = prop.totalGlobalMem;
    FY_HIP(hipStreamCreateWithFlags(&c->c.stream, hipStreamNonBlocking));
    fy::load_tuning_from_env(c->c.tune);
    *out = c.release();
    FY_CATCH
}

void fy_context_destroy(fy_context* c) {
    if (!c) return;
    (void)hipSetDevice(c->c.device);
    if (c->c.stream) {
        for (hipStream_t x : c->c.aux) (void)hipStreamSynchronize(x);   // lanes of a multi-cluster job (a failed job may have left work there)
        (void)hipStreamSynchronize(c->c.stream);
        c->c.trim();
        for (auto& kv : c->c.capacity) (void)hipFree(kv.first);   // blocks still held by live objects: caller error, reclaimed anyway
        c->c.capacity.clear();
        for (hipStream_t x : c->c.aux) { (void)hipStreamSynchronize(x); (void)hipStreamDestroy(x); }
        (void)hipStreamDestroy(c->c.stream);
    }
    delete c;
}

int fy_context_inject_alloc_failure(fy_context* c, int64_t nth) {
    if (!c || nth < 0) { set_error("context is NULL or nth < 0"); return FY_ERR_INVALID_ARGUMENT; }
    c->c.fail_alloc_in = nth;
    return FY_OK;
}

int fy_context_reload_tuning(fy_context* c) {
    if (!c) { set_error("context is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    fy::load_tuning_from_env(c->c.tune);
    return FY_OK;
}

int fy_context_synchronize(fy_context* c) {
    if (!c) { set_error("context is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(&c->c);
    FY_HIP(hipStreamSynchronize(c->c.stream));
    FY_CATCH
}

void* fy_context_stream(fy_context* c) { return c ? (void*)c->c.stream : nullptr; }

int fy_ratings_create(fy_context* c, int64_t nnz, const int32_t* user, const int32_t* item, const float* score, int location,
                      fy_ratings** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!c) { set_error("context is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (nnz < 0 || (nnz > 0 && (!user || !item || !score))) { set_error("ratings arrays are NULL or nnz < 0"); return FY_ERR_INVALID_ARGUMENT; }
    if (location != FY_HOST && location != FY_DEVICE) { set_error("location must be FY_HOST or FY_DEVICE"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    std::unique_ptr<fy_ratings> r(new fy_ratings);
    r->ctx = &c->c;
    r->nnz = nnz;
    r->user.alloc(&c->c, (size_t)nnz);
    r->item.alloc(&c->c, (size_t)nnz);
    r->score.alloc(&c->c, (size_t)nnz);
    if (nnz) {
        const hipMemcpyKind k = location == FY_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
        FY_HIP(hipMemcpyAsync(r->user.get(), user, (size_t)nnz * 4, k, c->c.stream));
        FY_HIP(hipMemcpyAsync(r->item.get(), item, (size_t)nnz * 4, k, c->c.stream));
        FY_HIP(hipMemcpyAsync(r->score.get(), score, (size_t)nnz * 4, k, c->c.stream));
        FY_HIP(hipStreamSynchronize(c->c.stream));   // the caller may free its arrays when this returns
        fy::ratings_id_bounds(&c->c, r.get());
    }
    *out = r.release();
    FY_CATCH
}

void fy_ratings_destroy(fy_ratings* r) {
    if (!r) return;
    fy::Context* ctx = r->ctx;
    if (ctx) (void)hipSetDevice(ctx->device);
    delete r;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
}
int64_t fy_ratings_nnz(const fy_ratings* r) { return r ? r->nnz : 0; }
void fy_ratings_drop_cache(fy_ratings* r) {
    if (!r) return;
    if (r->ctx) (void)hipSetDevice(r->ctx->device);
    std::shared_ptr<void> old;
    {
        std::lock_guard<std::mutex> g(r->cache_mu);
        old.swap(r->rm2_cache);
    }
    if (old && r->ctx) (void)hipStreamSynchronize(r->ctx->stream);     // nothing queued may still read what is released next
    old.reset();
}

int fy_ratings_apply(fy_context* c, const fy_ratings* r, int64_t n, const int32_t* user, const int32_t* item, const float* score,
                     const uint8_t* remove_or_null, int location, fy_ratings** out, fy_ratings_update_stats* stats_or_null) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (n < 0 || (n > 0 && (!user || !item || !score))) { set_error("write arrays are NULL or n < 0"); return FY_ERR_INVALID_ARGUMENT; }
    if (location != FY_HOST && location != FY_DEVICE) { set_error("location must be FY_HOST or FY_DEVICE"); return FY_ERR_INVALID_ARGUMENT; }
    if (!c || !r) { set_error("context or ratings is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->ctx != &c->c) { set_error("ratings belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    *out = fy::ratings_apply(&c->c, r, n, user, item, score, remove_or_null, location, stats_or_null);
    FY_CATCH
}

int fy_ratings_copy_out(const fy_ratings* r, int32_t* user, int32_t* item, float* score) {
    if (!r) { set_error("ratings is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->nnz > 0 && (!user || !item || !score)) { set_error("output arrays are NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->nnz == 0) return FY_OK;
    FY_TRY
    select_device(r->ctx);
    fy::d2h(r->ctx, user, r->user.get(), (size_t)r->nnz);
    fy::d2h(r->ctx, item, r->item.get(), (size_t)r->nnz);
    fy::d2h(r->ctx, score, r->score.get(), (size_t)r->nnz);
    fy::sync(r->ctx);
    FY_CATCH
}

// ---------------------------------------------------------------- RM2
int fy_rm2_prepare(fy_context* c, const fy_rm2_params* p, const fy_ratings* r, int64_t n_map, const int32_t* map_user,
                   const int32_t* map_cluster, const int32_t* cluster_count, fy_rm2_job** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!c || !r) { set_error("context or ratings is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->ctx != &c->c) { set_error("ratings belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    *out = fy::rm2_prepare(&c->c, p, r, n_map, map_user, map_cluster, cluster_count);
    {
        std::lock_guard<std::mutex> g(g_jobs_mu);
        g_jobs[*out] = &c->c;
    }
    FY_CATCH
}

int fy_rm2_partial_stats(fy_rm2_job* j, double** device_buf, int64_t* len) {
    if (!j || !device_buf || !len) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(job_context(j));
    fy::rm2_partial_stats(j, device_buf, len);
    FY_CATCH
}

int fy_rm2_stats_layout(fy_rm2_job* j, int64_t* n_item_slots, int64_t* n_user_slots) {
    if (!j || !n_item_slots || !n_user_slots) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    fy::rm2_stats_layout(j, n_item_slots, n_user_slots);
    FY_CATCH
}

int fy_rm2_set_global_stats(fy_rm2_job* j, const double* gathered_device, int32_t world) {
    if (!j || !gathered_device) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(job_context(j));
    fy::rm2_set_global_stats(j, gathered_device, world);
    FY_CATCH
}

int fy_rm2_set_collectives(fy_rm2_job* j, const fy_collectives* c) {
    if (!j || !c) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    fy::rm2_set_collectives(j, c);
    FY_CATCH
}

int fy_rm2_score(fy_rm2_job* j, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!j) { set_error("job is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(job_context(j));
    *out = fy::rm2_score(j);
    FY_CATCH
}

int fy_rm2_score_users(fy_rm2_job* j, const fy_rm2_request* rq, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!j || !rq) { set_error("job or request is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (rq->n_users < 0 || (rq->n_users > 0 && !rq->users)) { set_error("users is NULL or n_users < 0"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(job_context(j));
    *out = fy::rm2_score_users(j, rq);
    FY_CATCH
}

int fy_rm2_score_profiles(fy_rm2_job* j, const fy_rm2_profiles* profiles, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!j || !profiles) { set_error("job or profiles is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(job_context(j));
    *out = fy::rm2_score_profiles(j, profiles);
    FY_CATCH
}

void fy_rm2_job_destroy(fy_rm2_job* j) {
    if (!j) return;
    fy::Context* ctx = nullptr;
    {
        std::lock_guard<std::mutex> g(g_jobs_mu);
        auto it = g_jobs.find(j);
        if (it != g_jobs.end()) { ctx = it->second; g_jobs.erase(it); }
    }
    if (ctx) (void)hipSetDevice(ctx->device);
    fy::rm2_job_destroy(j);
}

int fy_rm2_run(const fy_rm2_params* p, int64_t nnz, const int32_t* user, const int32_t* item, const float* score, int64_t n_map,
               const int32_t* map_user, const int32_t* map_cluster, const int32_t* cluster_count, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    fy_context* c = nullptr;
    fy_ratings* r = nullptr;
    fy_rm2_job* j = nullptr;
    int rc = fy_context_create(0, &c);
    if (rc == FY_OK) rc = fy_ratings_create(c, nnz, user, item, score, FY_HOST, &r);
    if (rc == FY_OK) rc = fy_rm2_prepare(c, p, r, n_map, map_user, map_cluster, cluster_count, &j);
    if (rc == FY_OK) rc = fy_rm2_score(j, out);
    if (rc == FY_OK) {
        // the result outlives the context: bring everything to the host now
        (void)fy_result_key0(*out);
        (void)fy_result_user_sum(*out);
        (*out)->d_key0.release(); (*out)->d_key1.release(); (*out)->d_aux.release(); (*out)->d_value.release();
        (*out)->d_user_id.release(); (*out)->d_item_id.release(); (*out)->d_user_sum.release(); (*out)->d_icoll.release();
        (*out)->ctx = nullptr;
    }
    fy_rm2_job_destroy(j);
    fy_ratings_destroy(r);
    fy_context_destroy(c);
    return rc;
}

// ---------------------------------------------------------------- item-item similarity
int fy_itemsim_build(fy_context* c, const fy_itemsim_params* p, const fy_ratings* r, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!c || !r || !p) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->ctx != &c->c) { set_error("ratings belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    *out = fy::itemsim_build(&c->c, p, r);
    FY_CATCH
}

int fy_itemsim_run(const fy_itemsim_params* p, int64_t nnz, const int32_t* user, const int32_t* item, const float* score,
                   fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    fy_context* c = nullptr;
    fy_ratings* r = nullptr;
    int rc = fy_context_create(0, &c);
    if (rc == FY_OK) rc = fy_ratings_create(c, nnz, user, item, score, FY_HOST, &r);
    if (rc == FY_OK) rc = fy_itemsim_build(c, p, r, out);
    if (rc == FY_OK) {
        (void)fy_result_key0(*out);
        (*out)->d_key0.release(); (*out)->d_key1.release(); (*out)->d_aux.release(); (*out)->d_value.release();
        (*out)->ctx = nullptr;
    }
    fy_ratings_destroy(r);
    fy_context_destroy(c);
    return rc;
}

int fy_itemsim_prepare(fy_context* c, const fy_itemsim_params* p, const fy_ratings* r, fy_itemsim_job** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!c || !r || !p) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->ctx != &c->c) { set_error("ratings belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    *out = fy::itemsim_prepare(&c->c, p, r);
    FY_CATCH
}

int fy_itemsim_rows(fy_itemsim_job* j, const fy_itemsim_request* rq, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!j || !rq) { set_error("job or request is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (rq->n_items < 0 || (rq->n_items > 0 && !rq->items)) { set_error("items is NULL or n_items < 0"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(j->ctx);
    *out = fy::itemsim_rows(j, rq);
    FY_CATCH
}

void fy_itemsim_job_destroy(fy_itemsim_job* j) {
    if (!j) return;
    fy::Context* ctx = j->ctx;
    if (ctx) (void)hipSetDevice(ctx->device);
    delete j;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
}

int fy_cluster_assign(fy_context* c, int32_t n_rows, int32_t k, const double* H, int location, int32_t first_user,
                      int32_t cluster_offset, int32_t n_clusters, int32_t* user_out, int32_t* cluster_out, int32_t* count_inout) {
    if (!c) { set_error("context is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    fy::cluster_assign(&c->c, n_rows, k, H, location, first_user, cluster_offset, n_clusters, user_out, cluster_out, count_inout);
    FY_CATCH
}

int fy_nmf_factorize(fy_context* c, const fy_nmf_params* p, const fy_ratings* r, double* H, double* W, fy_stats* st) {
    if (!c || !r) { set_error("context or ratings is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->ctx != &c->c) { set_error("ratings belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    fy::nmf_factorize(&c->c, p, r, H, W, st);
    FY_CATCH
}

int fy_itemcf_recommend(fy_context* c, const fy_itemcf_params* p, const fy_ratings* r, fy_result* sims, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!c || !r || !p || !sims) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->ctx != &c->c || sims->ctx != &c->c) { set_error("ratings / similarities belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    if (sims->kind != 1) { set_error("`similarities` is not the result of fy_itemsim_build"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    *out = fy::itemcf_recommend(&c->c, p, r, sims);
    FY_CATCH
}

int fy_itemcf_recommend_filtered(fy_context* c, const fy_itemcf_params* p, const fy_itemcf_filter* f, const fy_ratings* r,
                                 fy_result* sims, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!c || !r || !p || !f || !sims) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->ctx != &c->c || sims->ctx != &c->c) { set_error("ratings / similarities belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    if (sims->kind != 1) { set_error("`similarities` is not the result of fy_itemsim_build"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    *out = fy::itemcf_recommend_filtered(&c->c, p, f, r, sims);
    FY_CATCH
}

int fy_itemcf_recommend_prepared(fy_itemsim_job* j, const fy_itemcf_params* p, const fy_itemcf_filter* f, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!j || !p) { set_error("job or parameters are NULL"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(j->ctx);
    *out = fy::itemcf_recommend_prepared(j, p, f);
    FY_CATCH
}

int fy_itemcf_recommend_profiles(fy_itemsim_job* j, const fy_itemcf_params* p, const fy_itemcf_profiles* profiles, const fy_itemcf_filter* items_only,
                                 fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!j || !p || !profiles) { set_error("job, parameters or profiles are NULL"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(j->ctx);
    *out = fy::itemcf_recommend_profiles(j, p, profiles, items_only);
    FY_CATCH
}

int fy_itemcf_estimate_prepared(fy_itemsim_job* j, const fy_itemcf_params* p, const fy_itemcf_pairs* pairs, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!j || !p || !pairs) { set_error("job, parameters or pairs are NULL"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(j->ctx);
    *out = fy::itemcf_estimate_prepared(j, p, pairs->n_pairs, pairs->users, pairs->items, pairs->location);
    FY_CATCH
}

int fy_itemcf_estimate_ratings(fy_itemsim_job* j, const fy_itemcf_params* p, const fy_ratings* asked, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!j || !p || !asked) { set_error("job, parameters or ratings are NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (asked->ctx != j->ctx) { set_error("the asked ratings belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(j->ctx);
    *out = fy::itemcf_estimate_prepared(j, p, asked->nnz, asked->user.get(), asked->item.get(), FY_DEVICE);
    FY_CATCH
}

int fy_itemcf_because_prepared(fy_itemsim_job* j, const fy_itemcf_params* p, const fy_itemcf_pairs* pairs, int32_t how_many, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!j || !p || !pairs) { set_error("job, parameters or pairs are NULL"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(j->ctx);
    *out = fy::itemcf_because_prepared(j, p, pairs->n_pairs, pairs->users, pairs->items, pairs->location, how_many);
    FY_CATCH
}

void fy_itemsim_job_drop_rows(fy_itemsim_job* j) {
    if (!j) return;
    if (j->ctx) (void)hipSetDevice(j->ctx->device);
    fy::itemsim_job_drop_rows(j);
}

int fy_ratings_shifted(fy_context* c, const fy_ratings* r, float shift, fy_ratings** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!c || !r) { set_error("context or ratings is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->ctx != &c->c) { set_error("ratings belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    *out = fy::ratings_shifted(&c->c, r, shift);
    FY_CATCH
}

int fy_itemsim_pairs(fy_context* c, fy_result* sims, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!c || !sims) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (sims->ctx != &c->c) { set_error("similarities belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    if (sims->kind != 1) { set_error("`similarities` is not the result of fy_itemsim_build"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    *out = fy::itemsim_pairs(&c->c, sims);
    FY_CATCH
}

// ---------------------------------------------------------------- offline evaluation
int fy_ratings_holdout(fy_context* c, const fy_ratings* r, double fraction, uint64_t seed, fy_ratings** train, fy_ratings** test) {
    if (train) *train = nullptr;
    if (test) *test = nullptr;
    if (!train || !test) { set_error("train or test is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (!c || !r) { set_error("context or ratings is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->ctx != &c->c) { set_error("ratings belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    fy::ratings_holdout(&c->c, r, fraction, seed, train, test);
    FY_CATCH
}

int fy_result_create_lists(fy_context* c, int64_t n, const int32_t* user, const int32_t* item, const float* value, int location, fy_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!c) { set_error("context is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (n < 0 || (n > 0 && (!user || !item || !value))) { set_error("row arrays are NULL or n < 0"); return FY_ERR_INVALID_ARGUMENT; }
    if (location != FY_HOST && location != FY_DEVICE) { set_error("location must be FY_HOST or FY_DEVICE"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    *out = fy::result_create_lists(&c->c, n, user, item, value, location);
    FY_CATCH
}

int fy_eval_prepare(fy_context* c, const fy_eval_params* p, const fy_ratings* test, fy_eval** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!c || !p || !test) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (test->ctx != &c->c) { set_error("ratings belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    *out = fy::eval_prepare(&c->c, p, test);
    FY_CATCH
}

int fy_eval_lists(fy_eval* e, fy_result* lists, fy_eval_sums* out, int32_t* per_user_id_or_null, double* per_user_or_null) {
    if (!e || !lists || !out) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (lists->ctx != e->ctx) { set_error("the lists belong to another context (or live on the host only)"); return FY_ERR_INVALID_ARGUMENT; }
    if (lists->kind != 0 && lists->kind != 2) { set_error("not a list result: item similarities and item pairs cannot be evaluated"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(e->ctx);
    fy::eval_lists(e, lists, out, per_user_id_or_null, per_user_or_null);
    FY_CATCH
}

int fy_eval_estimates(fy_context* c, fy_result* estimates, const fy_ratings* truth, const fy_eval_error_params* params_or_null, fy_eval_errors* out) {
    if (!c || !estimates || !truth || !out) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (estimates->ctx != &c->c || truth->ctx != &c->c) { set_error("estimates / truth belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    if (estimates->kind != 4) { set_error("not a result of fy_itemcf_estimate_prepared / fy_itemcf_estimate_ratings"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    fy::eval_estimates(&c->c, estimates, truth, params_or_null, out);
    FY_CATCH
}

void fy_eval_destroy(fy_eval* e) {
    if (!e) return;
    fy::Context* ctx = e->ctx;
    if (ctx) (void)hipSetDevice(ctx->device);
    delete e;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
}

// ---------------------------------------------------------------- results
static void rows_to_host(fy_result* r) {
    if (r->rows_on_host) return;
    r->rows_on_host = true;
    const size_t n = (size_t)r->n;
    r->h_key0.resize(n); r->h_key1.resize(n); r->h_aux.resize(n); r->h_value.resize(n);
    if (n == 0 || !r->ctx) return;
    try {
        select_device(r->ctx);
        fy::d2h(r->ctx, r->h_key0.data(), r->d_key0.get(), n);
        fy::d2h(r->ctx, r->h_key1.data(), r->d_key1.get(), n);
        fy::d2h(r->ctx, r->h_aux.data(), r->d_aux.get(), n);
        fy::d2h(r->ctx, r->h_value.data(), r->d_value.get(), n);
        fy::sync(r->ctx);
    } catch (const fy::Failure&) {
    }
}
static void sums_to_host(fy_result* r) {
    if (r->sums_on_host) return;
    r->sums_on_host = true;
    const size_t nu = r->d_user_id.size(), ni = r->d_item_id.size();
    r->h_user_id.resize(nu); r->h_user_sum.resize(nu); r->h_item_id.resize(ni); r->h_icoll.resize(ni);
    if (!r->ctx) return;
    try {
        select_device(r->ctx);
        fy::d2h(r->ctx, r->h_user_id.data(), r->d_user_id.get(), nu);
        fy::d2h(r->ctx, r->h_user_sum.data(), r->d_user_sum.get(), nu);
        fy::d2h(r->ctx, r->h_item_id.data(), r->d_item_id.get(), ni);
        if (r->d_icoll.size() == ni) fy::d2h(r->ctx, r->h_icoll.data(), r->d_icoll.get(), ni);
        fy::sync(r->ctx);
    } catch (const fy::Failure&) {
    }
}

int64_t fy_result_size(fy_result* r) { return r ? r->n : 0; }
const int32_t* fy_result_key0(fy_result* r) { if (!r) return nullptr; rows_to_host(r); return r->h_key0.data(); }
const int32_t* fy_result_key1(fy_result* r) { if (!r) return nullptr; rows_to_host(r); return r->h_key1.data(); }
const float* fy_result_value(fy_result* r) { if (!r) return nullptr; rows_to_host(r); return r->h_value.data(); }
const int32_t* fy_result_aux(fy_result* r) { if (!r) return nullptr; rows_to_host(r); return r->h_aux.data(); }
int64_t fy_result_n_users(fy_result* r) { if (!r) return 0; sums_to_host(r); return (int64_t)r->h_user_id.size(); }
const int32_t* fy_result_user_id(fy_result* r) { if (!r) return nullptr; sums_to_host(r); return r->h_user_id.data(); }
const double* fy_result_user_sum(fy_result* r) { if (!r) return nullptr; sums_to_host(r); return r->h_user_sum.data(); }
int64_t fy_result_n_items(fy_result* r) { if (!r) return 0; sums_to_host(r); return (int64_t)r->h_item_id.size(); }
const int32_t* fy_result_item_id(fy_result* r) { if (!r) return nullptr; sums_to_host(r); return r->h_item_id.data(); }
const double* fy_result_item_coll(fy_result* r) { if (!r) return nullptr; sums_to_host(r); return r->h_icoll.data(); }
double fy_result_total_sum(fy_result* r) { return r ? r->total_sum : 0.0; }
int fy_result_stats(fy_result* r, fy_stats* out) {
    if (!r || !out) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    *out = r->st;
    return FY_OK;
}
int fy_result_request_stats(fy_result* r, fy_rm2_request_stats* out) {
    if (!r || !out) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (!r->has_request_stats) { set_error("not a result of fy_rm2_score_users"); return FY_ERR_STATE; }
    *out = r->rq;
    return FY_OK;
}
int fy_result_rm2_profile_stats(fy_result* r, fy_rm2_profile_stats* out) {
    if (!r || !out) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (!r->has_rm2_profile_stats) { set_error("not a result of fy_rm2_score_profiles"); return FY_ERR_STATE; }
    *out = r->rpf;
    return FY_OK;
}
int fy_result_itemsim_request_stats(fy_result* r, fy_itemsim_request_stats* out) {
    if (!r || !out) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (!r->has_itemsim_request_stats) { set_error("not a result of fy_itemsim_rows"); return FY_ERR_STATE; }
    *out = r->irq;
    return FY_OK;
}
int fy_result_itemcf_request_stats(fy_result* r, fy_itemcf_request_stats* out) {
    if (!r || !out) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (!r->has_itemcf_request_stats) { set_error("not a result of fy_itemcf_recommend_prepared"); return FY_ERR_STATE; }
    *out = r->crq;
    return FY_OK;
}
int fy_result_itemcf_profile_stats(fy_result* r, fy_itemcf_profile_stats* out) {
    if (!r || !out) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (!r->has_itemcf_profile_stats) { set_error("not a result of fy_itemcf_recommend_profiles"); return FY_ERR_STATE; }
    *out = r->cpf;
    return FY_OK;
}
int fy_result_itemcf_estimate_stats(fy_result* r, fy_itemcf_estimate_stats* out) {
    if (!r || !out) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (!r->has_itemcf_estimate_stats) { set_error("not a result of fy_itemcf_estimate_prepared / fy_itemcf_estimate_ratings"); return FY_ERR_STATE; }
    *out = r->est;
    return FY_OK;
}
int fy_result_itemcf_because_stats(fy_result* r, fy_itemcf_because_stats* out) {
    if (!r || !out) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (!r->has_itemcf_because_stats) { set_error("not a result of fy_itemcf_because_prepared"); return FY_ERR_STATE; }
    *out = r->bec;
    return FY_OK;
}
// the per-pair arrays and the per-row preference of an explanations result, on the host from the first call on
static int because_to_host(fy_result* r) {
    if (r->because_on_host) return FY_OK;
    FY_TRY
    const size_t np = (size_t)r->bp_n, n = (size_t)r->n;
    std::vector<int32_t> start32(np + 1, 0);
    r->h_bp_user.resize(np); r->h_bp_item.resize(np); r->h_bp_status.resize(np); r->h_bp_cnt.resize(np); r->h_bp_est.resize(np);
    r->h_bp_start.assign(np + 1, 0);
    r->h_pref.resize(n);
    if (np > 0 && r->ctx) {
        select_device(r->ctx);
        fy::d2h(r->ctx, r->h_bp_user.data(), r->d_bp_user.get(), np);
        fy::d2h(r->ctx, r->h_bp_item.data(), r->d_bp_item.get(), np);
        fy::d2h(r->ctx, r->h_bp_status.data(), r->d_bp_status.get(), np);
        fy::d2h(r->ctx, r->h_bp_cnt.data(), r->d_bp_cnt.get(), np);
        fy::d2h(r->ctx, r->h_bp_est.data(), r->d_bp_est.get(), np);
        fy::d2h(r->ctx, start32.data(), r->d_bp_start.get(), np + 1);
        fy::d2h(r->ctx, r->h_pref.data(), r->d_pref.get(), n);
        fy::sync(r->ctx);
    }
    for (size_t t = 0; t <= np; t++) r->h_bp_start[t] = start32[t];
    r->because_on_host = true;
    FY_CATCH
}
int fy_result_because_view(fy_result* r, fy_itemcf_because_view* out) {
    if (!r || !out) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (!r->has_itemcf_because_stats) { set_error("not a result of fy_itemcf_because_prepared"); return FY_ERR_STATE; }
    const int rc = because_to_host(r);
    if (rc != FY_OK) return rc;
    out->n_pairs = r->bp_n;
    out->start = r->h_bp_start.data();
    out->user = r->h_bp_user.data();
    out->item = r->h_bp_item.data();
    out->estimate = r->h_bp_est.data();
    out->status = r->h_bp_status.data();
    out->contributors = r->h_bp_cnt.data();
    out->pref = r->h_pref.data();
    return FY_OK;
}
void fy_result_free(fy_result* r) {
    if (!r) return;
    fy::Context* ctx = r->ctx;
    if (ctx) (void)hipSetDevice(ctx->device);
    delete r;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
}

// ---- fold-in (fy_foldin.hip)
int fy_foldin_create(fy_context* c, const fy_foldin_params* p, const double* W, int location, const int32_t* count, int64_t n_count, fy_foldin** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!p) { set_error("params is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (p->number_of_items <= 0 || p->number_of_clusters <= 0) { set_error("numberOfItems / numberOfClusters must be > 0"); return FY_ERR_INVALID_ARGUMENT; }
    if (p->number_of_clusters > 256) { set_error("numberOfClusters %d exceeds the kernel limit 256", p->number_of_clusters); return FY_ERR_UNSUPPORTED; }
    if (!W) { set_error("W is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (location != FY_HOST && location != FY_DEVICE) { set_error("location must be FY_HOST or FY_DEVICE"); return FY_ERR_INVALID_ARGUMENT; }
    if (n_count < 0 || (n_count > 0 && !count)) { set_error("count is NULL with n_count > 0, or n_count < 0"); return FY_ERR_INVALID_ARGUMENT; }
    if (!c) { set_error("context is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    FY_HIP(hipSetDevice(c->c.device));
    *out = fy::foldin_create(&c->c, p, W, location, count, n_count);
    FY_CATCH
}
int fy_foldin_add_level(fy_foldin* f, int32_t n_parents, const int32_t* items_in_cluster, const int32_t* sub_clusters, const int32_t* item_raw,
                        const double* W_ragged, int32_t stride, const int32_t* count, int64_t n_count) {
    if (!f) { set_error("the fold-in model is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(f->ctx);
    fy::foldin_add_level(f, n_parents, items_in_cluster, sub_clusters, item_raw, W_ragged, stride, count, n_count);
    FY_CATCH
}
int fy_foldin_assign(fy_foldin* f, const fy_itemcf_profiles* profiles, int32_t iterations, int32_t first_iteration, const double* h0, int32_t rank,
                     int32_t world, fy_foldin_result** out) {
    if (!out) { set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!f || !profiles) { set_error("the fold-in model or the profiles are NULL"); return FY_ERR_INVALID_ARGUMENT; }
    FY_TRY
    select_device(f->ctx);
    *out = fy::foldin_assign(f, profiles, iterations, first_iteration, h0, rank, world);
    FY_CATCH
}
int64_t fy_foldin_result_n(const fy_foldin_result* r) { return r ? (int64_t)r->label.size() : 0; }
int64_t fy_foldin_result_sub_size(const fy_foldin_result* r) { return r ? r->sub_off.back() : 0; }
int fy_foldin_result_assignment(const fy_foldin_result* r, int32_t* label, int32_t* cluster, int32_t* parent, int32_t* status) {
    if (!r || (!r->label.empty() && (!label || !cluster || !parent || !status))) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    const size_t b = r->label.size() * sizeof(int32_t);
    if (b) { memcpy(label, r->label.data(), b); memcpy(cluster, r->cluster.data(), b); memcpy(parent, r->parent.data(), b); memcpy(status, r->status.data(), b); }
    return FY_OK;
}
int fy_foldin_result_factors(fy_foldin_result* r, double* H) {
    if (!r || (!r->label.empty() && !H)) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->label.empty()) return FY_OK;
    FY_TRY
    select_device(r->ctx);
    fy::d2h(r->ctx, H, r->H.get(), r->label.size() * (size_t)r->k);
    fy::sync(r->ctx);
    FY_CATCH
}
int fy_foldin_result_sub_factors(fy_foldin_result* r, int64_t* offset, double* H) {
    if (!r || !offset || (r->sub_off.back() > 0 && !H)) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    memcpy(offset, r->sub_off.data(), r->sub_off.size() * sizeof(int64_t));
    if (r->sub_off.back() == 0) return FY_OK;
    FY_TRY
    select_device(r->ctx);
    fy::d2h(r->ctx, H, r->H1.get(), (size_t)r->sub_off.back());
    fy::sync(r->ctx);
    FY_CATCH
}
int fy_foldin_result_stats(const fy_foldin_result* r, fy_foldin_stats* out) {
    if (!r || !out) { set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    *out = r->stats;
    return FY_OK;
}
void fy_foldin_result_free(fy_foldin_result* r) {
    if (!r) return;
    fy::Context* ctx = r->ctx;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    delete r;
}
void fy_foldin_destroy(fy_foldin* f) {
    if (!f) return;
    fy::Context* ctx = f->ctx;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    delete f;
}

}  // extern "C"
