// fy_itemcf_request.hip -- item-based CF on request from a prepared similarity job (fy_itemcf_recommend_prepared).
//
// DESIGN.md section 2d.  A user's prediction needs the similarity rows of that user's own maxPrefsPerUser strongest preferences and
// nothing else of the matrix, and the prepared job (fy_itemsim_job) builds any row on request.  The job's Prepared IS the structure
// the filtered pass (icf_run, fy_itemcf.hip) sorts out of the ratings, so nothing here sorts or walks the ratings:
//   users -> slot list      one binary search per requested id (k_icfr_find_users), ordered / deduplicated on the host (<= n ids)
//   thresholds              k_icf_threshold<true> of the filtered pass
//   k_icfr_mark_items       one wave per listed user: every kept preference (p >= thr) sets its column's bit -- the set J
//   k_icfr_split            J against the job's row store: needed / missing per column; the missing ones are compacted (scan) into
//                           an ascending rank list
//   rows                    the request row kernel + merge of fy_itemsim_request.hip over the missing ranks (itemsim_build_rank_rows)
//   k_icfr_fill_store       one wave per built row: the row into the store (other item as a column, similarity), THEN its count and
//                           its state -- a row is present only once it is complete
//   accumulate .. compact   icf_score_lists of the filtered pass with row_start[j] = j * K and row_cnt read from the store
// The per-cell order of additions is the order of the user's preferences, as in the filtered pass, so the result is the filtered
// pass's bit for bit when it is fed the rows fy_itemsim_rows returns; the store changes where a row comes from, never its bits.
// The steps from the thresholds to k_icfr_fill_store are icfr_rows_for_users, which the profile pass (fy_itemcf_profiles.hip) and the
// passes over named pairs (fy_itemcf_pairs.hip) call too: a row built for any pass serves the others.  The frame every such pass
// shares is here as well: the result (icfr_new_result, icfr_no_rows, icfr_nobody), the list pass over the store
// (icfr_lists_from_store) and the fy_stats (icfr_finish_stats).
#include <algorithm>
#include <limits>

#include "fy_itemcf_request.hpp"

namespace fy {
namespace {

// requested raw user id -> (slot << 32 | dense index), or all ones for an id nobody has
__global__ void k_icfr_find_users(int64_t n, const int32_t* __restrict__ ids, const int32_t* __restrict__ uid, int32_t nU,
                                  const int32_t* __restrict__ du2slot, uint64_t* __restrict__ found) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t du = icf_find_user(uid, nU, ids[t]);
        found[t] = du >= 0 ? (((uint64_t)(uint32_t)du2slot[du] << 32) | (uint32_t)du) : ~0ull;
    }
}

// one wave per listed user lo .. hi: the columns of its kept preferences (what k_icf_accumulate does not skip) -> bitmap
__global__ void k_icfr_mark_items(int32_t lo, int32_t hi, const int32_t* __restrict__ list, const int32_t* __restrict__ rowptr,
                                  const int32_t* __restrict__ csr_idx, const float* __restrict__ csr_r, const float* __restrict__ thr,
                                  int32_t n_cols, uint32_t* __restrict__ need) {
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int32_t k = lo + blockIdx.x * wpb + (threadIdx.x >> 6); k < hi; k += gridDim.x * wpb) {
        const int32_t s = list[k];
        const float t = thr[k - lo];
        for (int32_t f = rowptr[s] + lane; f < rowptr[s + 1]; f += 64) {
            if (csr_r[f] < t) continue;
            const int32_t j = csr_idx[f];
            if (j >= 0 && j < n_cols) atomicOr(&need[j >> 5], 1u << (j & 31));
        }
    }
}

// per column: needed by the request?  already in the store?  missing[c] = needed and not stored; *n_needed = needed columns
__global__ void k_icfr_split(int32_t n_cols, const uint32_t* __restrict__ need, const int32_t* __restrict__ state,
                             int32_t* __restrict__ missing, int32_t* __restrict__ n_needed) {
    int32_t mine = 0;
    for (int32_t c = blockIdx.x * blockDim.x + threadIdx.x; c <= n_cols; c += gridDim.x * blockDim.x) {
        const bool needed = c < n_cols && ((need[c >> 5] >> (c & 31)) & 1u);
        missing[c] = needed && state[c] == 0;      // (missing[n_cols] = 0: the scan's total lands there)
        mine += needed;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_needed, mine);
}

__global__ void k_icfr_list_missing(int32_t n_cols, const int32_t* __restrict__ missing, const int32_t* __restrict__ pos,
                                    int32_t* __restrict__ rows) {
    for (int32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n_cols; c += gridDim.x * blockDim.x)
        if (missing[c]) rows[pos[c]] = c;
}

__global__ void k_icfr_row_starts(int32_t n_cols, int32_t K, int32_t* __restrict__ start) {
    for (int32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n_cols; c += gridDim.x * blockDim.x) start[c] = c * K;
}

// one wave per built row m (popularity rank rows[m]): its merged list -> the store, the other item re-expressed as a column as
// k_icf_index_sims does; the count and the state are written by the wave that wrote the entries, after them
__global__ void k_icfr_fill_store(int32_t n, int32_t K, int32_t n_cols, const int32_t* __restrict__ rows, const int32_t* __restrict__ cnt,
                                  const int32_t* __restrict__ other, const float* __restrict__ sim, const int32_t* __restrict__ iid,
                                  int32_t nI, const int32_t* __restrict__ pair_rank, int32_t* __restrict__ s_state,
                                  int32_t* __restrict__ s_cnt, int32_t* __restrict__ s_other, float* __restrict__ s_sim) {
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int32_t m = blockIdx.x * wpb + (threadIdx.x >> 6); m < n; m += gridDim.x * wpb) {
        const int32_t r = rows[m];
        if (r < 0 || r >= n_cols) continue;
        const int32_t c = min(cnt[m], K);
        for (int32_t i = lane; i < c; i += 64) {
            s_other[(int64_t)r * K + i] = icf_column(iid, nI, pair_rank, other[(int64_t)m * K + i]);
            s_sim[(int64_t)r * K + i] = sim[(int64_t)m * K + i];
        }
        __threadfence();
        if (lane == 0) {
            s_cnt[r] = c;
            s_state[r] = 1;
        }
    }
}

}  // namespace

void itemsim_job_drop_rows(fy_itemsim_job* J) { J->store = fy_itemsim_job::RowStore{}; }

void icfr_check_job(const fy_itemsim_job* J) {
    if (J->prm.world != 1) FY_FAIL(FY_ERR_UNSUPPORTED, "the similarity job was prepared as rank %d of %d: every rank needs any row (prepare with world = 1)", J->prm.rank, J->prm.world);
    if (J->prm.min_prefs_per_user > 1 || J->prm.max_prefs_per_user != 0)
        FY_FAIL(FY_ERR_UNSUPPORTED, "the similarity job was prepared with minPrefsPerUser / maxPrefsPerUser: its rows are no longer the users' preferences");
}

void icfr_check_store(const fy_itemsim_job* J) {
    if ((int64_t)J->P.nP * J->prm.max_similarities_per_item > (int64_t)std::numeric_limits<int32_t>::max())
        FY_FAIL(FY_ERR_UNSUPPORTED, "the row store would exceed 2^31 entries");
}

void icfr_rows_for_users(fy_itemsim_job* J, const IcfRowView& V, const int32_t* list, int32_t lo, int32_t hi, int32_t max_prefs, float* thr, IcfrTimers& tm,
                         size_t sp_tab, IcfrRows& rq) {
    Context* ctx = J->ctx;
    const Prepared& P = J->P;
    const int32_t K = J->prm.max_similarities_per_item, nP = P.nP, nmine = hi - lo;
    hipStream_t st = ctx->stream;
    std::vector<int32_t> h_missing;
    int32_t h_need = 0, h_build = 0;
    SyncOnUnwind drain(st);      // behind the host ends of the queued copies; the scratch buffers below go back to the allocator before it drains
    icf_thresholds(ctx, V, list, lo, hi, max_prefs, thr);

    // ---- the row store of the job, on the first call: every buffer or none
    fy_itemsim_job::RowStore& store = J->store;
    if (!store.allocated) {
        fy_itemsim_job::RowStore fresh;
        fresh.state.alloc(ctx, (size_t)nP);
        fresh.cnt.alloc(ctx, (size_t)nP);
        fresh.start.alloc(ctx, (size_t)nP);
        fresh.other.alloc(ctx, (size_t)nP * K);
        fresh.sim.alloc(ctx, (size_t)nP * K);
        fresh.state.zero();
        fresh.cnt.zero();
        k_icfr_row_starts<<<grid_for(nP), 256, 0, st>>>(nP, K, fresh.start.get());
        FY_KERNEL_CHECK();
        fresh.allocated = true;
        store = std::move(fresh);
    }

    // ---- J: the columns of the kept preferences; those the store lacks, ascending
    DevBuf<uint32_t> need(ctx, (size_t)ceil_div(nP, 32));
    DevBuf<int32_t> missing(ctx, (size_t)nP + 1), pos(ctx, (size_t)nP + 1), n_needed(ctx, 1);
    need.zero();
    n_needed.zero();
    k_icfr_mark_items<<<grid_for((int64_t)nmine * 64, 256), 256, 0, st>>>(lo, hi, list, V.rowptr, V.csr_idx, V.csr_r, thr, nP, need.get());
    FY_KERNEL_CHECK();
    k_icfr_split<<<grid_for((int64_t)nP + 1), 256, 0, st>>>(nP, need.get(), store.state.get(), missing.get(), n_needed.get());
    FY_KERNEL_CHECK();
    exclusive_scan_i32(ctx, missing.get(), pos.get(), (size_t)nP + 1);
    d2h(ctx, &h_need, n_needed.get(), 1);
    d2h(ctx, &h_build, pos.get() + nP, 1);      // the scan's total: the missing columns
    sync(ctx);
    const int64_t n_need = h_need, n_build = h_build;
    rq.items_needed = n_need;
    rq.rows_built = n_build;
    rq.rows_from_store = n_need - n_build;
    DevBuf<int32_t> rows(ctx, (size_t)n_build);
    if (n_build > 0) {
        k_icfr_list_missing<<<grid_for(nP), 256, 0, st>>>(nP, missing.get(), pos.get(), rows.get());
        FY_KERNEL_CHECK();
        h_missing.resize((size_t)n_build);
        d2h(ctx, h_missing.data(), rows.get(), (size_t)n_build);
    }
    tm.tables.end(sp_tab);

    // ---- build the missing rows and keep them
    if (n_build > 0) {
        DevBuf<int32_t> cnt(ctx, (size_t)n_build), other(ctx, (size_t)n_build * K);
        DevBuf<float> sim(ctx, (size_t)n_build * K);
        rq.batches = itemsim_build_rank_rows(J, rows.get(), n_build, cnt.get(), other.get(), sim.get(), tm.cooc, tm.cooc);
        const size_t sp_f = tm.cooc.begin();
        k_icfr_fill_store<<<grid_for(n_build * 64, 256), 256, 0, st>>>((int32_t)n_build, K, nP, rows.get(), cnt.get(), other.get(), sim.get(), P.iid.get(),
                                                                      P.nI, P.pair_rank.get(), store.state.get(), store.cnt.get(), store.other.get(),
                                                                      store.sim.get());
        FY_KERNEL_CHECK();
        tm.cooc.end(sp_f);
        store.rows += n_build;
        sync(ctx);      // the list of the built rows is on the host
        for (int32_t r : h_missing) rq.pair_contribs += J->walk[(size_t)r];
    }
    rq.rows_stored = store.rows;
}

std::unique_ptr<fy_result> icfr_new_result(const fy_itemsim_job* J, int kind) {
    std::unique_ptr<fy_result> Rs(new fy_result);
    Rs->ctx = J->ctx;
    Rs->kind = kind;
    Rs->st.nnz = J->P.nnz;
    Rs->st.n_users = J->P.nU;
    Rs->st.n_items = J->P.nI;
    Rs->d_user_id.alloc(J->ctx, 0);
    Rs->d_item_id.alloc(J->ctx, 0);
    return Rs;
}

fy_result* icfr_no_rows(std::unique_ptr<fy_result> Rs) {
    Rs->d_key0.alloc(Rs->ctx, 0);
    Rs->d_key1.alloc(Rs->ctx, 0);
    Rs->d_value.alloc(Rs->ctx, 0);
    Rs->d_aux.alloc(Rs->ctx, 0);
    return Rs.release();
}

void icfr_finish_stats(fy_result* Rs, const IcfrRows& built, int64_t users_scored, int64_t score_launches, IcfrTimers& tm) {
    Rs->st.recs = Rs->n;
    Rs->st.users_scored = users_scored;
    Rs->st.pair_contribs = built.pair_contribs;
    Rs->st.cooc_launches = built.batches;
    Rs->st.score_launches = score_launches;
    Rs->st.ms_tables = tm.tables.total_ms();
    Rs->st.ms_cooc = tm.cooc.total_ms();
    Rs->st.ms_score = tm.score.total_ms();
    Rs->st.ms_topn = tm.topn.total_ms();
    Rs->st.ms_total = tm.total.total_ms();
}

fy_result* icfr_nobody(std::unique_ptr<fy_result> Rs, IcfrTimers& tm, size_t sp_tab, size_t sp_total) {
    tm.tables.end(sp_tab);
    tm.total.end(sp_total);
    sync(Rs->ctx);
    icfr_finish_stats(Rs.get(), IcfrRows{}, 0, 0, tm);
    return icfr_no_rows(std::move(Rs));
}

int64_t icfr_lists_from_store(fy_itemsim_job* J, const fy_itemcf_params* prm, const IcfRowView& V, const int32_t* list, const int32_t* list_du,
                              const uint32_t* allow, int32_t lo, int32_t hi, const float* thr, const IcfrRows& built, fy_result* Rs, IcfrTimers& tm,
                              size_t sp_total) {
    Context* ctx = J->ctx;
    const fy_itemsim_job::RowStore& store = J->store;
    DevBuf<int32_t> n_lists;
    const IcfSims S{store.start.get(), store.cnt.get(), store.other.get(), store.sim.get()};
    icf_score_lists(ctx, prm, V, S, list, list_du, allow, lo, hi, thr, Rs, tm.score, tm.topn, n_lists);
    tm.total.end(sp_total);
    const int64_t scored = (int64_t)fetch(ctx, n_lists.get());
    sync(ctx);
    icfr_finish_stats(Rs, built, scored, (int64_t)tm.score.count(), tm);
    return scored;
}

fy_result* itemcf_recommend_prepared(fy_itemsim_job* J, const fy_itemcf_params* prm, const fy_itemcf_filter* filt) {
    Context* ctx = J->ctx;
    const Prepared& P = J->P;
    if (!filt || !filt->has_users)
        FY_FAIL(FY_ERR_INVALID_ARGUMENT, "fy_itemcf_recommend_prepared needs the users to recommend for (has_users); lists for every user are fy_itemcf_recommend's");
    icf_check_arguments(prm, filt);
    icfr_check_job(J);
    hipStream_t st = ctx->stream;
    std::unique_ptr<fy_result> Rs = icfr_new_result(J, 2);
    Rs->has_itemcf_request_stats = true;
    fy_itemcf_request_stats& rq = Rs->crq;
    rq.users_asked = filt->n_users;
    rq.rows_stored = J->store.rows;
    // Mahout's empty id set: nobody is asked for / nothing may be recommended
    if (P.nnz == 0 || filt->n_users == 0 || (filt->has_items && filt->n_items == 0)) return icfr_no_rows(std::move(Rs));
    icfr_check_store(J);

    IcfrTimers tm(ctx);
    std::vector<uint64_t> found((size_t)filt->n_users);
    std::vector<int32_t> slots, dus;
    // behind the host ends of the queued copies (and the caller's id arrays).  The scratch buffers below are declared after it and so
    // go back to the allocator BEFORE a failure drains the stream, as in icf_run: the allocator hands blocks out again on this same
    // stream only, and no later call queues work before this one has unwound.
    SyncOnUnwind drain(st);
    const size_t sp_total = tm.total.begin();
    const size_t sp_tab = tm.tables.begin();
    // ---- the request: known users once each, in slot order -- the list of the filtered pass
    {
        DevBuf<int32_t> ids(ctx, (size_t)filt->n_users);
        DevBuf<uint64_t> d_found(ctx, (size_t)filt->n_users);
        h2d(ctx, ids.get(), filt->users, (size_t)filt->n_users);
        k_icfr_find_users<<<grid_for(filt->n_users), 256, 0, st>>>(filt->n_users, ids.get(), P.uid.get(), P.nU, P.du2slot.get(), d_found.get());
        FY_KERNEL_CHECK();
        d2h(ctx, found.data(), d_found.get(), (size_t)filt->n_users);
        sync(ctx);
    }
    std::sort(found.begin(), found.end());
    found.erase(std::unique(found.begin(), found.end()), found.end());
    while (!found.empty() && found.back() == ~0ull) found.pop_back();
    const int32_t n_all = (int32_t)found.size();
    // this rank's users: a contiguous range of the list, as in the filtered pass
    int32_t lo = 0, hi = n_all;
    if (prm->world > 1) {
        lo = (int32_t)((int64_t)n_all * prm->rank / prm->world);
        hi = (int32_t)((int64_t)n_all * (prm->rank + 1) / prm->world);
    }
    const int32_t nmine = hi - lo;
    rq.users_known = nmine;
    if (nmine == 0) return icfr_nobody(std::move(Rs), tm, sp_tab, sp_total);
    slots.resize((size_t)n_all);
    dus.resize((size_t)n_all);
    for (int32_t k = 0; k < n_all; k++) {
        slots[(size_t)k] = (int32_t)(found[(size_t)k] >> 32);
        dus[(size_t)k] = (int32_t)(uint32_t)found[(size_t)k];
    }
    DevBuf<int32_t> list(ctx, (size_t)n_all), list_du(ctx, (size_t)n_all);
    DevBuf<uint32_t> allow;
    h2d(ctx, list.get(), slots.data(), (size_t)n_all);
    h2d(ctx, list_du.get(), dus.data(), (size_t)n_all);
    if (filt->has_items) icf_allow_bitmap(ctx, P, filt, allow);
    DevBuf<float> thr(ctx, (size_t)nmine + 1);
    // ---- thresholds, the set J, the rows the store lacks: built and kept
    IcfrRows built;
    const IcfRowView V = icf_rows_of(P);
    icfr_rows_for_users(J, V, list.get(), lo, hi, prm->max_prefs_per_user, thr.get(), tm, sp_tab, built);
    icfr_report(rq, built, true);

    // ---- accumulate, finalize, top-N, compact: the filtered pass, reading the store
    icfr_lists_from_store(J, prm, V, list.get(), list_du.get(), filt->has_items ? allow.get() : nullptr, lo, hi, thr.get(), built, Rs.get(), tm, sp_total);
    return Rs.release();
}

}  // namespace fy
