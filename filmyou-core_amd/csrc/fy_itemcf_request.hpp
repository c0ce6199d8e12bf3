// fy_itemcf_request.hpp -- item-based CF on request from a prepared similarity job (fy_itemcf_recommend_prepared:
// fy_itemcf_request.hip) and the steps of the filtered pass it shares with fy_itemcf.hip.
#pragma once
#include "fy_itemsim_request.hpp"

namespace fy {

// raw item id -> compact column (popularity rank); -1 when the item has no rating
__device__ __forceinline__ int32_t icf_column(const int32_t* __restrict__ iid, int32_t nI, const int32_t* __restrict__ pair_rank, int32_t raw) {
    int32_t lo = 0, hi = nI;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (iid[mid] < raw) lo = mid + 1; else hi = mid;
    }
    return (lo < nI && iid[lo] == raw) ? pair_rank[lo] : -1;
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
void icf_thresholds(Context*, const Prepared&, const int32_t* list, int32_t lo, int32_t hi, int32_t max_prefs, float* thr);
// Batches of users with dense accumulators: accumulate, finalize, top-N, and the compaction of the lists into Rs (n, rows).
// list / list_du == nullptr: the unrestricted pass over the slots lo .. hi; allow == nullptr: every item.  n_lists (the list pass
// only) is left holding the number of users that received a list.
void icf_score_lists(Context*, const fy_itemcf_params*, const Prepared&, const IcfSims&, const int32_t* list, const int32_t* list_du,
                     const uint32_t* allow, int32_t lo, int32_t hi, const float* thr, fy_result* Rs, EventTimer& t_score, EventTimer& t_topn,
                     DevBuf<int32_t>& n_lists);

fy_result* itemcf_recommend_prepared(fy_itemsim_job*, const fy_itemcf_params*, const fy_itemcf_filter*);
void itemsim_job_drop_rows(fy_itemsim_job*);

}  // namespace fy
