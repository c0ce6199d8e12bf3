// fy_itemcf_pairs.hpp -- what the two passes that answer named (user, item) PAIRS on a prepared similarity job share: the estimates
// (fy_itemcf_estimate.hip) and the explanations (fy_itemcf_because.hip).  The host steps and their kernels are fy_itemcf_pairs.hip;
// each pass keeps its own checks, buffers, kernel and statistics.  Here: their declarations, the arguments both kernels take, and
// the finish of a cell, which both kernels call so that (estimate, status) cannot differ between them.
#pragma once
#include "fy_itemcf_request.hpp"

namespace fy {

// What the front half leaves for the pass's own kernel.
struct IcfPairTargets {
    DevBuf<int32_t> own_users, own_items;   // host pairs: their copy in HBM
    const int32_t *d_users = nullptr, *d_items = nullptr;   // this rank's pairs in HBM
    int32_t n_known = 0;                    // distinct known users = length of `list`
    int32_t n_targets = 0;                  // distinct (known user, known item) pairs
    DevBuf<int32_t> pslot, upos, list;      // per pair: slot; per slot: position in `list`; the known users' slots, ascending
    DevBuf<float> thr;                      // by position in `list`
    IcfrRows built;
    DevBuf<uint32_t> splace;                // place in the input of every sorted entry
    DevBuf<uint64_t> tkey;                  // n_targets
    DevBuf<int32_t> tfirst;                 // n_targets + 1
};

// The arguments k_icf_estimate and k_icf_because share.  The arrays are the base of both kernels' structs; K, boolean_data, tkey,
// tfirst and splace are common too but stay members of EstArgs / BecArgs, between each kernel's own fields: with all thirteen in the
// base the arguments lie at other offsets and both kernels measured 2 - 3 % slower (profiles/itemcf_request_frame/README.md).
// icf_pair_args fills the thirteen.
struct IcfPairArgs {
    const int32_t* __restrict__ rowptr;
    const int32_t* __restrict__ csr_idx;
    const float* __restrict__ csr_r;
    const float* __restrict__ thr;          // by position in the slot list
    const int32_t* __restrict__ list;       // slot of the user at a position
    const int32_t* __restrict__ row_cnt;    // the job's row store: row j = entries j * K .. + row_cnt[j]
    const int32_t* __restrict__ col_other;
    const float* __restrict__ sim;
};

// The finish of a cell as k_icf_finalize (fy_itemcf.hip) does it, with the reason when there is no value: returns the status and
// leaves v the estimate or NaN.  own: the item is one of the user's kept preferences.
__device__ __forceinline__ int32_t icf_estimate_finish(double num, double den, int32_t cnt, bool own, int32_t boolean_data, float& v) {
    v = __builtin_nanf("");
    if (own) return FY_ESTIMATE_OWN_PREFERENCE;
    if (boolean_data ? cnt < 1 : cnt < 2) return FY_ESTIMATE_TOO_FEW;
    if (!(num != 0.0)) return FY_ESTIMATE_ZERO_NUMERATOR;
    v = boolean_data ? (float)num : (float)(num / den);
    return v == v ? FY_ESTIMATE_OK : FY_ESTIMATE_NOT_A_NUMBER;
}

// The opening of either pass behind its own argument checks: rank / world, the pair list and its location, the 2^31 bounds, what
// the job must be and that its store fits; off / n = this rank's contiguous range of the pair list; the result of `kind`.
std::unique_ptr<fy_result> icf_pairs_open(fy_itemsim_job* J, const fy_itemcf_params* prm, int64_t n_all_pairs, const int32_t* users, const int32_t* items,
                                          int location, int kind, int64_t& off, int32_t& n);

// The rank's n pairs (users / items: already offset to the range; location FY_HOST / FY_DEVICE) -> the row of every pair as far as
// the key pass knows it (o_*: n each), the rows of the kept preferences of the known users in J->store, the targets:
//   k_est_find_users     per pair: the user's slot (icf_find_user), a flag per slot; scan + k_est_list_users: the known users once
//                        each in slot order -- the slot list icfr_rows_for_users (fy_itemcf_request.hip) takes, as the list pass does
//   icfr_rows_for_users  thresholds, the set J, the rows the job's store lacks: built and kept (shared with the list pass)
//   k_est_keys           per pair: (position of the user in the slot list << 32 | column of the item) and its place in the input;
//                        an unknown user / item gets its row here and an all-ones key
//   sort                 rocPRIM radix sort of (key, place): equal keys are one TARGET, a user's targets are adjacent, columns ascending
//   heads, targets       key and first sorted entry of every target
// The caller has begun span sp_tab of tm.tables; it is ended and begun again around the row build (icfr_rows_for_users) and is OPEN
// on return: the caller ends it behind its own table work.  Synchronises.
void icf_pair_targets(fy_itemsim_job* J, int32_t max_prefs, int32_t n, const int32_t* users, const int32_t* items, int location, int32_t* o_user,
                      int32_t* o_item, float* o_value, int32_t* o_aux, IcfrTimers& tm, size_t& sp_tab, IcfPairTargets& T, const char* what);

template <class Args>      // EstArgs or BecArgs
inline void icf_pair_args(Args& A, const fy_itemsim_job* J, const IcfPairTargets& T, int32_t boolean_data) {
    const Prepared& P = J->P;
    const fy_itemsim_job::RowStore& store = J->store;
    A.rowptr = P.rowptr.get(); A.csr_idx = P.csr_idx.get(); A.csr_r = P.csr_r.get();
    A.thr = T.thr.get(); A.list = T.list.get();
    A.row_cnt = store.cnt.get(); A.col_other = store.other.get(); A.sim = store.sim.get();
    A.K = J->prm.max_similarities_per_item; A.boolean_data = boolean_data;
    A.tkey = T.tkey.get(); A.tfirst = T.tfirst.get(); A.splace = T.splace.get();
}

// The closing of either pass: the rows per status of aux[0 .. n) into agg[0 .. 7], the end of span sp_total, agg on the host (h_agg:
// agg.size() sums, [8] = the users with an OK pair), by_status[0 .. 7], the fy_stats.  Synchronises.
void icf_pairs_close(fy_result* Rs, int32_t n, const int32_t* aux, DevBuf<unsigned long long>& agg, unsigned long long* h_agg, int64_t* by_status,
                     const IcfrRows& built, int64_t score_launches, IcfrTimers& tm, size_t sp_total);

}  // namespace fy
