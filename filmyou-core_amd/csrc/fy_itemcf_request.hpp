// fy_itemcf_request.hpp -- item-based CF on request from a prepared similarity job (fy_itemcf_recommend_prepared:
// fy_itemcf_request.hip), the steps of the filtered pass it shares with fy_itemcf.hip, and the frame (result, row build, statistics)
// that every pass over a prepared job's rows shares.
#pragma once
#include "fy_itemsim_request.hpp"

namespace fy {

// raw item id -> compact column (popularity rank); -1 when the item has no rating
__device__ __forceinline__ int32_t icf_column(const int32_t* __restrict__ iid, int32_t nI, const int32_t* __restrict__ pair_rank, int32_t raw) {
    const int32_t lo = fy_lower_bound(iid, 0, nI, raw);
    return (lo < nI && iid[lo] == raw) ? pair_rank[lo] : -1;
}

// dense index of a raw user id among the nU ascending ids, -1 for an id nobody has
__device__ __forceinline__ int32_t icf_find_user(const int32_t* __restrict__ uid, int32_t nU, int32_t raw) {
    const int32_t lo = fy_lower_bound(uid, 0, nU, raw);
    return (lo < nU && uid[lo] == raw) ? lo : -1;
}

// The users' rows as the list pass reads them: row s = entries rowptr[s] .. rowptr[s + 1] of csr_idx (columns, ascending inside a row) /
// csr_r (preferences); a row is named uid[slot2du[s]] in the result, and column c is the raw item rank_item_raw[c] of n_cols.  The
// resident callers pass the job's own arrays (icf_rows_of); the profile pass (fy_itemcf_profiles.hip) passes the CSR it composed, with
// the profiles' labels as uid.
struct IcfRowView {
    const int32_t* rowptr;
    const int32_t* csr_idx;
    const float* csr_r;
    const int32_t* uid;
    const int32_t* slot2du;
    const int32_t* rank_item_raw;
    int32_t n_cols;
};
inline IcfRowView icf_rows_of(const Prepared& P) {
    return IcfRowView{P.rowptr.get(), P.csr_idx.get(), P.csr_r.get(), P.uid.get(), P.slot2du.get(), P.rank_item_raw.get(), P.nP};
}

// the similarity rows as k_icf_accumulate reads them: row j = entries row_start[j] .. + row_cnt[j] of col_other / sim
struct IcfSims {
    const int32_t* row_start;
    const int32_t* row_cnt;
    const int32_t* col_other;
    const float* sim;
};

// ---- steps of icf_run (fy_itemcf.hip), each with the launches it had there
// numRecommendations / maxPrefsPerUser / (rank, world) of the parameters and the arrays of the filter: the pass's own failures
void icf_check_arguments(const fy_itemcf_params*, const fy_itemcf_filter*);
// itemsFile: the allowed raw item ids -> bitmap over the columns
void icf_allow_bitmap(Context*, const Prepared&, const fy_itemcf_filter*, DevBuf<uint32_t>& allow);
// thr[k - lo] for the users lo .. hi of the slot list (list == nullptr: slots lo .. hi)
void icf_thresholds(Context*, const IcfRowView&, const int32_t* list, int32_t lo, int32_t hi, int32_t max_prefs, float* thr);
// Batches of users with dense accumulators: accumulate, finalize, top-N, and the compaction of the lists into Rs (n, rows).
// list / list_du == nullptr: the unrestricted pass over the slots lo .. hi; allow == nullptr: every item.  n_lists (the list pass
// only) is left holding the number of users that received a list.
void icf_score_lists(Context*, const fy_itemcf_params*, const IcfRowView&, const IcfSims&, const int32_t* list, const int32_t* list_du,
                     const uint32_t* allow, int32_t lo, int32_t hi, const float* thr, fy_result* Rs, EventTimer& t_score, EventTimer& t_topn,
                     DevBuf<int32_t>& n_lists);

// ---- the frame of a pass that reads a prepared job's rows (fy_itemcf_request.hip): the two list passes (fy_itemcf_recommend_prepared
// there, fy_itemcf_recommend_profiles in fy_itemcf_profiles.hip) and the two passes over named pairs (the estimates,
// fy_itemcf_estimate.hip, and the explanations, fy_itemcf_because.hip; what those two share beyond it is fy_itemcf_pairs.hip)
// what the job must be to serve either (world == 1, no minPrefsPerUser / maxPrefsPerUser of its own), and that its store fits
void icfr_check_job(const fy_itemsim_job*);
// a result of `kind` on the job's context: the job's three counts in its fy_stats, no id tables
std::unique_ptr<fy_result> icfr_new_result(const fy_itemsim_job*, int kind);
// the result without rows (where there are lists, icf_score_lists allocates the four columns)
fy_result* icfr_no_rows(std::unique_ptr<fy_result> Rs);
// the phase timers of a pass; one that never begins a span costs nothing and reads 0 ms
struct IcfrTimers {
    EventTimer total, tables, cooc, score, topn;
    explicit IcfrTimers(Context* c) : total(c), tables(c), cooc(c), score(c), topn(c) {}
};
struct IcfrRows {
    int64_t items_needed = 0, rows_built = 0, rows_from_store = 0, rows_stored = 0, pair_contribs = 0, batches = 0;
};
// what icfr_rows_for_users did, into the pass's own statistics.  built_any == false: no user was known and the row builder never
// ran, so rows_stored stays the count the pass read at entry.
template <class S>
inline void icfr_report(S& s, const IcfrRows& b, bool built_any) {
    s.items_needed = b.items_needed;
    s.rows_built = b.rows_built;
    s.rows_from_store = b.rows_from_store;
    if (built_any) s.rows_stored = b.rows_stored;
    s.pair_contribs = b.pair_contribs;
    s.batches = b.batches;
}
// the fy_stats of a pass whose stream has been synchronised behind the end of tm.total; recs = the rows of the result
void icfr_finish_stats(fy_result* Rs, const IcfrRows& built, int64_t users_scored, int64_t score_launches, IcfrTimers& tm);
// nobody is left to score behind the pass's own table work: the two open spans end, the result without rows
fy_result* icfr_nobody(std::unique_ptr<fy_result> Rs, IcfrTimers& tm, size_t sp_tab, size_t sp_total);
// Rows lo .. hi of the view, their rows in the job's store: icf_score_lists, the end of span sp_total, the fy_stats.  Synchronises.
// Returns the number of users that received a list.
int64_t icfr_lists_from_store(fy_itemsim_job* J, const fy_itemcf_params* prm, const IcfRowView& V, const int32_t* list, const int32_t* list_du,
                              const uint32_t* allow, int32_t lo, int32_t hi, const float* thr, const IcfrRows& built, fy_result* Rs, IcfrTimers& tm,
                              size_t sp_total);
// For the rows lo .. hi of the list (device; slots of the job's own rows, or rows of a composed view): thr[k - lo] (hi - lo + 1 floats of the caller), the set J of
// their kept preferences, J against the job's row store (allocated here on the first call), the missing rows built and kept.  The
// caller has begun span sp_tab of tm.tables (its own id -> slot work is inside it); it is ended here, in front of the row build,
// whose spans go to tm.cooc.  Synchronises.  When it returns, row j of every kept preference is in J->store.
void icfr_rows_for_users(fy_itemsim_job* J, const IcfRowView& V, const int32_t* list, int32_t lo, int32_t hi, int32_t max_prefs, float* thr, IcfrTimers& tm,
                         size_t sp_tab, IcfrRows& out);

constexpr int ICF_EST_CHUNK_MAX = 512;   // FY_ICF_EST_CHUNK: targets a wave of the estimate kernel holds in LDS (4 waves x 28 B x 512 = 56 KiB)
fy_result* itemcf_recommend_prepared(fy_itemsim_job*, const fy_itemcf_params*, const fy_itemcf_filter*);
// the 2^31-entry bound of the job's row store (FY_ERR_UNSUPPORTED), checked before the first row is asked for
void icfr_check_store(const fy_itemsim_job*);
// users / items: the whole pair list, n raw ids each, host or device (location); the rank's range is cut inside
fy_result* itemcf_estimate_prepared(fy_itemsim_job*, const fy_itemcf_params*, int64_t n, const int32_t* users, const int32_t* items, int location);
// the contributing preferences of the same pairs, at most how_many listed per pair (fy_itemcf_because.hip)
fy_result* itemcf_because_prepared(fy_itemsim_job*, const fy_itemcf_params*, int64_t n, const int32_t* users, const int32_t* items, int location,
                                   int32_t how_many);
void itemsim_job_drop_rows(fy_itemsim_job*);

}  // namespace fy
