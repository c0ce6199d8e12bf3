// fy_itemcf_pairs.hip -- the host frame and the front half of the passes over named (user, item) pairs on a prepared similarity
// job (fy_itemcf_pairs.hpp says who calls what): the opening, the steps from the pairs to the targets with their kernels, the common
// kernel arguments, the closing with the status count.  DESIGN.md sections 2f / 2h.
#include <limits>

#include "fy_itemcf_pairs.hpp"

namespace fy {
namespace {

constexpr uint64_t EST_NO_KEY = ~0ull;

// pair t: the slot of its user (-1: nobody has the id) and that slot's flag
__global__ void k_est_find_users(int64_t n, const int32_t* __restrict__ users, const int32_t* __restrict__ uid, int32_t nU,
                                 const int32_t* __restrict__ du2slot, int32_t* __restrict__ pslot, int32_t* __restrict__ flag) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t du = icf_find_user(uid, nU, users[t]);
        int32_t s = -1;
        if (du >= 0) {
            s = du2slot[du];
            flag[s] = 1;                                         // (every writer stores the same word)
        }
        pslot[t] = s;
    }
}

__global__ void k_est_list_users(int32_t nU, const int32_t* __restrict__ flag, const int32_t* __restrict__ pos, int32_t* __restrict__ list) {
    for (int32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nU; s += gridDim.x * blockDim.x)
        if (flag[s]) list[pos[s]] = s;
}

// The row of every pair as far as it is known here, its sort key and its place.  pslot == nullptr: a job over no preferences.
__global__ void k_est_keys(int64_t n, const int32_t* __restrict__ users, const int32_t* __restrict__ items, const int32_t* __restrict__ pslot,
                           const int32_t* __restrict__ pos, const int32_t* __restrict__ iid, int32_t nI, const int32_t* __restrict__ pair_rank,
                           uint64_t* __restrict__ keys, uint32_t* __restrict__ place, int32_t* __restrict__ o_user, int32_t* __restrict__ o_item,
                           float* __restrict__ o_value, int32_t* __restrict__ o_aux) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t it = items[t];
        const int32_t slot = pslot ? pslot[t] : -1;
        const int32_t col = slot >= 0 ? icf_column(iid, nI, pair_rank, it) : -1;
        o_user[t] = users[t];
        o_item[t] = it;
        o_value[t] = __builtin_nanf("");
        o_aux[t] = slot < 0 ? FY_ESTIMATE_UNKNOWN_USER : col < 0 ? FY_ESTIMATE_UNKNOWN_ITEM : FY_ESTIMATE_OK;      // (OK: the pass's own kernel writes the row)
        if (keys) {
            keys[t] = col >= 0 ? (((uint64_t)(uint32_t)pos[slot] << 32) | (uint32_t)col) : EST_NO_KEY;
            place[t] = (uint32_t)t;
        }
    }
}

// sorted keys: head[t] = first entry of a target; n_valid[0] = entries in front of the all-ones keys
__global__ void k_est_heads(int32_t n, const uint64_t* __restrict__ skeys, uint32_t* __restrict__ head, int32_t* __restrict__ n_valid) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        const bool valid = skeys[t] != EST_NO_KEY;
        head[t] = valid && (t == 0 || skeys[t] != skeys[t - 1]);
        if (valid && (t == n - 1 || skeys[t + 1] == EST_NO_KEY)) n_valid[0] = t + 1;
    }
}
// tkey[m], tfirst[m] = key and first sorted entry of target m; tfirst[targets] = n_valid
__global__ void k_est_targets(int32_t n_valid, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ head,
                              const uint32_t* __restrict__ head_incl, uint64_t* __restrict__ tkey, int32_t* __restrict__ tfirst) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_valid; t += gridDim.x * blockDim.x) {
        if (head[t]) {
            tkey[head_incl[t] - 1] = skeys[t];
            tfirst[head_incl[t] - 1] = t;
        }
        if (t == n_valid - 1) tfirst[head_incl[t]] = n_valid;
    }
}

// rows per status
__global__ void k_est_count_status(int64_t n, const int32_t* __restrict__ aux, unsigned long long* __restrict__ agg) {
    unsigned long long mine[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t s = aux[t] & 7;
#pragma unroll
        for (int q = 0; q < 8; q++) mine[q] += s == q;
    }
#pragma unroll
    for (int q = 0; q < 8; q++) {
        unsigned long long v = mine[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&agg[q], v);
    }
}

}  // namespace

std::unique_ptr<fy_result> icf_pairs_open(fy_itemsim_job* J, const fy_itemcf_params* prm, int64_t n_all_pairs, const int32_t* users, const int32_t* items,
                                          int location, int kind, int64_t& off, int32_t& n) {
    if (prm->world <= 0 || prm->rank < 0 || prm->rank >= prm->world) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "rank %d of world %d", prm->rank, prm->world);
    if (n_all_pairs < 0 || (n_all_pairs > 0 && (!users || !items))) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "users / items is NULL or n_pairs < 0");
    if (location != FY_HOST && location != FY_DEVICE) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "location must be FY_HOST or FY_DEVICE");
    if (n_all_pairs > (int64_t)std::numeric_limits<int32_t>::max()) FY_FAIL(FY_ERR_UNSUPPORTED, "%lld pairs: at most 2^31 - 1", (long long)n_all_pairs);
    icfr_check_job(J);
    icfr_check_store(J);
    // this rank's pairs: a contiguous range of the pair list
    off = n_all_pairs * prm->rank / prm->world;
    n = (int32_t)(n_all_pairs * (prm->rank + 1) / prm->world - off);
    return icfr_new_result(J, kind);
}

void icf_pair_targets(fy_itemsim_job* J, int32_t max_prefs, int32_t n, const int32_t* users, const int32_t* items, int location, int32_t* o_user,
                      int32_t* o_item, float* o_value, int32_t* o_aux, IcfrTimers& tm, size_t& sp_tab, IcfPairTargets& T, const char* what) {
    Context* ctx = J->ctx;
    const Prepared& P = J->P;
    hipStream_t st = ctx->stream;
    T.d_users = users;
    T.d_items = items;
    if (location == FY_HOST) {
        T.own_users.alloc(ctx, (size_t)n);
        T.own_items.alloc(ctx, (size_t)n);
        h2d(ctx, T.own_users.get(), users, (size_t)n);
        h2d(ctx, T.own_items.get(), items, (size_t)n);
        T.d_users = T.own_users.get();
        T.d_items = T.own_items.get();
    }
    // ---- the known users of the range once each, in slot order
    int32_t n_known = 0;
    if (P.nnz > 0) {
        DevBuf<int32_t> flag(ctx, (size_t)P.nU + 1);
        T.pslot.alloc(ctx, (size_t)n);
        T.upos.alloc(ctx, (size_t)P.nU + 1);
        flag.zero();
        k_est_find_users<<<grid_for(n), 256, 0, st>>>(n, T.d_users, P.uid.get(), P.nU, P.du2slot.get(), T.pslot.get(), flag.get());
        FY_KERNEL_CHECK();
        exclusive_scan_i32(ctx, flag.get(), T.upos.get(), (size_t)P.nU + 1);
        n_known = fetch(ctx, T.upos.get() + P.nU);
        if (n_known < 0 || n_known > P.nU) FY_FAIL(FY_ERR_HIP, "%s: %d known users of %d", what, n_known, P.nU);
        if (n_known > 0) {
            T.list.alloc(ctx, (size_t)n_known);
            k_est_list_users<<<grid_for(P.nU), 256, 0, st>>>(P.nU, flag.get(), T.upos.get(), T.list.get());
            FY_KERNEL_CHECK();
        }
    }
    T.n_known = n_known;
    T.n_targets = 0;
    if (n_known == 0) {
        // nobody is known: every row is written by the key pass
        k_est_keys<<<grid_for(n), 256, 0, st>>>(n, T.d_users, T.d_items, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, o_user, o_item, o_value, o_aux);
        FY_KERNEL_CHECK();
        return;
    }
    // ---- thresholds, the set J, the rows the store lacks: built and kept
    T.thr.alloc(ctx, (size_t)n_known + 1);
    icfr_rows_for_users(J, icf_rows_of(P), T.list.get(), 0, n_known, max_prefs, T.thr.get(), tm, sp_tab, T.built);

    // ---- pairs -> keys, sorted; targets
    sp_tab = tm.tables.begin();
    DevBuf<uint64_t> keys(ctx, (size_t)n), skeys(ctx, (size_t)n);
    DevBuf<uint32_t> place(ctx, (size_t)n), head(ctx, (size_t)n), head_incl(ctx, (size_t)n);
    DevBuf<int32_t> n_valid(ctx, 1);
    T.splace.alloc(ctx, (size_t)n);
    n_valid.zero();
    k_est_keys<<<grid_for(n), 256, 0, st>>>(n, T.d_users, T.d_items, T.pslot.get(), T.upos.get(), P.iid.get(), P.nI, P.pair_rank.get(), keys.get(), place.get(),
                                           o_user, o_item, o_value, o_aux);
    FY_KERNEL_CHECK();
    sort_pairs_u64_u32(ctx, keys.get(), skeys.get(), place.get(), T.splace.get(), (size_t)n);
    k_est_heads<<<grid_for(n), 256, 0, st>>>(n, skeys.get(), head.get(), n_valid.get());
    FY_KERNEL_CHECK();
    inclusive_scan_u32(ctx, head.get(), head_incl.get(), (size_t)n);
    int32_t h_valid = 0;
    uint32_t h_targets = 0;
    d2h(ctx, &h_valid, n_valid.get(), 1);
    d2h(ctx, &h_targets, head_incl.get() + (n - 1), 1);
    sync(ctx);
    const int32_t n_targets = (int32_t)h_targets;
    if (h_valid < 0 || h_valid > n || n_targets < 0 || n_targets > h_valid || (n_targets == 0) != (h_valid == 0))
        FY_FAIL(FY_ERR_HIP, "%s: %d targets in %d valid pairs of %d", what, n_targets, h_valid, n);
    T.n_targets = n_targets;
    if (n_targets > 0) {
        T.tkey.alloc(ctx, (size_t)n_targets);
        T.tfirst.alloc(ctx, (size_t)n_targets + 1);
        k_est_targets<<<grid_for(h_valid), 256, 0, st>>>(h_valid, skeys.get(), head.get(), head_incl.get(), T.tkey.get(), T.tfirst.get());
        FY_KERNEL_CHECK();
    }
}

void icf_pairs_close(fy_result* Rs, int32_t n, const int32_t* aux, DevBuf<unsigned long long>& agg, unsigned long long* h_agg, int64_t* by_status,
                     const IcfrRows& built, int64_t score_launches, IcfrTimers& tm, size_t sp_total) {
    Context* ctx = Rs->ctx;
    k_est_count_status<<<grid_for(n), 256, 0, ctx->stream>>>(n, aux, agg.get());
    FY_KERNEL_CHECK();
    tm.total.end(sp_total);
    d2h(ctx, h_agg, agg.get(), agg.size());
    sync(ctx);
    for (int q = 0; q < 8; q++) by_status[q] = (int64_t)h_agg[q];
    icfr_finish_stats(Rs, built, (int64_t)h_agg[8], score_launches, tm);
}

}  // namespace fy
