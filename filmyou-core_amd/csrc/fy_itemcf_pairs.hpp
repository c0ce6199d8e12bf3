// fy_itemcf_pairs.hpp -- the front half of the passes that answer named (user, item) PAIRS on a prepared similarity job: the
// estimates (fy_itemcf_estimate.hip) and the explanations (fy_itemcf_because.hip).  Both include it; every kernel here is
// file-local to the including translation unit.
//   k_est_find_users     per pair: the user's slot (binary search), a flag per slot; scan + k_est_list_users: the known users once
//                        each in slot order -- the slot list icfr_rows_for_users (fy_itemcf_request.hip) takes, as the list pass does
//   icfr_rows_for_users  thresholds, the set J, the rows the job's store lacks: built and kept (shared with the list pass)
//   k_est_keys           per pair: (position of the user in the slot list << 32 | column of the item) and its place in the input;
//                        an unknown user / item gets its row here and an all-ones key
//   sort                 rocPRIM radix sort of (key, place): equal keys are one TARGET, a user's targets are adjacent, columns ascending
//   heads, targets       key and first sorted entry of every target
#pragma once
#include "fy_itemcf_request.hpp"

namespace fy {

constexpr uint64_t EST_NO_KEY = ~0ull;

// pair t: the slot of its user (-1: nobody has the id) and that slot's flag
__attribute__((unused)) static __global__ void k_est_find_users(int64_t n, const int32_t* __restrict__ users, const int32_t* __restrict__ uid, int32_t nU,
                                 const int32_t* __restrict__ du2slot, int32_t* __restrict__ pslot, int32_t* __restrict__ flag) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t raw = users[t];
        int32_t lo = 0, hi = nU;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (uid[mid] < raw) lo = mid + 1; else hi = mid;
        }
        int32_t s = -1;
        if (lo < nU && uid[lo] == raw) {
            s = du2slot[lo];
            flag[s] = 1;                                         // (every writer stores the same word)
        }
        pslot[t] = s;
    }
}

__attribute__((unused)) static __global__ void k_est_list_users(int32_t nU, const int32_t* __restrict__ flag, const int32_t* __restrict__ pos, int32_t* __restrict__ list) {
    for (int32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nU; s += gridDim.x * blockDim.x)
        if (flag[s]) list[pos[s]] = s;
}

// The row of every pair as far as it is known here, its sort key and its place.  pslot == nullptr: a job over no preferences.
__attribute__((unused)) static __global__ void k_est_keys(int64_t n, const int32_t* __restrict__ users, const int32_t* __restrict__ items, const int32_t* __restrict__ pslot,
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
__attribute__((unused)) static __global__ void k_est_heads(int32_t n, const uint64_t* __restrict__ skeys, uint32_t* __restrict__ head, int32_t* __restrict__ n_valid) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        const bool valid = skeys[t] != EST_NO_KEY;
        head[t] = valid && (t == 0 || skeys[t] != skeys[t - 1]);
        if (valid && (t == n - 1 || skeys[t + 1] == EST_NO_KEY)) n_valid[0] = t + 1;
    }
}
// tkey[m], tfirst[m] = key and first sorted entry of target m; tfirst[targets] = n_valid
__attribute__((unused)) static __global__ void k_est_targets(int32_t n_valid, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ head,
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
__attribute__((unused)) static __global__ void k_est_count_status(int64_t n, const int32_t* __restrict__ aux, unsigned long long* __restrict__ agg) {
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

// The rank's n pairs (users / items: already offset to the range; location FY_HOST / FY_DEVICE) -> the row of every pair as far as
// the key pass knows it (o_*: n each), the rows of the kept preferences of the known users in J->store, the targets.  The caller
// has begun span sp_tab of t_tables; it is ended and begun again around the row build (icfr_rows_for_users) and is OPEN on return:
// the caller ends it behind its own table work.  Synchronises.
__attribute__((unused)) static void icf_pair_targets(fy_itemsim_job* J, int32_t max_prefs, int32_t n, const int32_t* users, const int32_t* items, int location,
                                                     int32_t* o_user, int32_t* o_item, float* o_value, int32_t* o_aux, EventTimer& t_tables, size_t& sp_tab,
                                                     EventTimer& t_cooc, IcfPairTargets& T, const char* what) {
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
    icfr_rows_for_users(J, icf_rows_of(P), T.list.get(), 0, n_known, max_prefs, T.thr.get(), t_tables, sp_tab, t_cooc, T.built);

    // ---- pairs -> keys, sorted; targets
    sp_tab = t_tables.begin();
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

}  // namespace fy
