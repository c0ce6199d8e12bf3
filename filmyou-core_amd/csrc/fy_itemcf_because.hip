// fy_itemcf_because.hip -- item-based CF: named (user, item) pairs explained by their contributing preferences on a prepared
// similarity job (fy_itemcf_because_prepared; include/filmyou.h).
//
// The explanation of (u, i) is the decomposition of the cell (u, i) that k_icf_estimate (fy_itemcf_estimate.hip) finishes: the terms
// pref * sim of the kept preferences j of u whose row holds i, the best how_many of them listed.  Opening, front half (user slots,
// the rows of the kept preferences in the job's store, keys, sort, targets) and closing are the estimates': fy_itemcf_pairs.hip.
//   k_icf_because   ONE WAVE per distinct target.  The wave walks the user's kept preferences in CSR order; for each j with a
//                   non-empty row the 64 lanes stride over the row's entries looking for column i.  A row holds a column at most
//                   once, so at most one lane hits; the hit becomes wave-uniform by ballot / readlane.  num, den (fp64) and cnt are
//                   wave-uniform and receive their additions in preference order exactly as k_icf_estimate's cells do: the rounded
//                   product __dmul_rn(pref, sim), then the rounded sums, then the one icf_estimate_finish -- so (estimate, status)
//                   are the estimates' bit for bit.
//                   The best how_many terms so far live ONE PER LANE in registers, sorted (NaN last, weight descending, raw id
//                   ascending): an insert is one compare on every lane, a ballot whose population count is the position, and a
//                   shift by one lane (__shfl_up).  No LDS, no atomics, no second walk; hence how_many <= 64.
//                   The wave writes its entries to a how_many-strided scratch and (estimate, status, cnt, listed, target) to every
//                   asked place of the target.
//   scan, compact   exclusive scan over the listed counts per asked pair; k_bec_compact copies every place's entries into the
//                   grouped rows.
// Nothing is sized by the catalogue.  Work model: fy_itemcf_because_stats.row_entries_walked (per target, not per chunk).
#include <limits>

#include "fy_itemcf_pairs.hpp"

namespace fy {
namespace {

constexpr int BEC_AGG = 11;      // status counts [0 .. 7], users with an OK pair [8], row entries walked [9], contributors over the asked pairs [10]

struct BecArgs : IcfPairArgs {                // (K .. splace: in both kernels' structs, at the offsets the kernels were tuned with)
    const int32_t* __restrict__ rank_item_raw;   // column -> raw item id
    int32_t K, boolean_data, n_targets, H;    // H = how_many
    const uint64_t* __restrict__ tkey;
    const int32_t* __restrict__ tfirst;       // targets + 1
    const uint32_t* __restrict__ splace;      // place in the input of every sorted entry
    int32_t* __restrict__ s_item;             // scratch, targets x H: the listed entries of a target, best first
    float* __restrict__ s_sim;
    float* __restrict__ s_pref;
    float* __restrict__ p_est;                // per asked pair
    int32_t* __restrict__ p_status;
    int32_t* __restrict__ p_cnt;
    int32_t* __restrict__ p_rows;
    int32_t* __restrict__ p_target;
    long long* __restrict__ walked;           // per target
    int32_t* __restrict__ user_ok;            // per position in the slot list: one of the user's targets is FY_ESTIMATE_OK
};

__global__ void __launch_bounds__(256) k_icf_because(BecArgs A) {
    const int lane = threadIdx.x & 63;
    const int32_t m = blockIdx.x * 4 + (__builtin_amdgcn_readfirstlane(threadIdx.x) >> 6);      // (wave-uniform, and known to be)
    if (m >= A.n_targets) return;                                // (no workgroup barrier below: the waves are independent)
    const uint64_t key = A.tkey[m];
    const int32_t k = (int32_t)(key >> 32), col = (int32_t)(uint32_t)key;
    const int32_t slot = A.list[k];
    const float thr = A.thr[k];
    double num = 0.0, den = 0.0;
    int32_t cnt = 0, own = 0, filled = 0;
    long long walked = 0;
    // this lane's entry of the sorted list (valid iff lane < filled)
    double e_w = 0.0;
    int32_t e_id = 0;
    float e_sim = 0.0f, e_pref = 0.0f;
    const int32_t f1 = A.rowptr[slot + 1];
    for (int32_t f = A.rowptr[slot]; f < f1; f++) {              // preferences in CSR order; everything but the search is wave-uniform
        const float p = A.csr_r[f];
        if (p < thr) continue;
        const int32_t j = A.csr_idx[f];
        const int32_t n = A.row_cnt[j];
        if (n == 0) continue;                                    // no similarity row: contributes nothing, not even its self entry (k_icf_estimate)
        walked += n;
        if (j == col) own = 1;                                   // the (j, NaN) self entry: the item itself drops out
        const int32_t t0 = j * A.K;
        unsigned long long hit = 0;
        float sv = 0.0f;
        for (int32_t base = 0; base < n && !hit; base += 64) {   // a row holds a column at most once: at most one lane hits
            const int32_t t = base + lane;
            const bool h = t < n && A.col_other[t0 + t] == col;
            if (h) sv = A.sim[t0 + t];
            hit = __ballot(h);
        }
        if (!hit) continue;
        const float sf = __shfl(sv, __ffsll((long long)hit) - 1, 64);
        const double s = (double)sf;
        const double pd = A.boolean_data ? 1.0 : (double)p;
        const double term = __dmul_rn(pd, s);
        num = __dadd_rn(num, term);
        den = __dadd_rn(den, fabs(s));
        cnt += 1;
        // ---- insert (term, id) into the sorted list: the entries that stay in front of it are a prefix of the lanes
        const int32_t id = A.rank_item_raw[j];
        const bool x_nan = term != term, e_nan = e_w != e_w;
        bool x_first;                                            // the new entry goes in front of this lane's
        if (x_nan != e_nan) x_first = e_nan;
        else if (!x_nan && term != e_w) x_first = term > e_w;
        else x_first = id < e_id;
        const int pos = __popcll(__ballot(lane < filled && !x_first));
        if (pos < A.H) {
            const double u_w = __shfl_up(e_w, 1, 64);
            const int32_t u_id = __shfl_up(e_id, 1, 64);
            const float u_sim = __shfl_up(e_sim, 1, 64), u_pref = __shfl_up(e_pref, 1, 64);
            if (lane > pos) {
                e_w = u_w; e_id = u_id; e_sim = u_sim; e_pref = u_pref;
            } else if (lane == pos) {
                e_w = term; e_id = id; e_sim = sf; e_pref = A.boolean_data ? 1.0f : p;
            }
            filled = min(filled + 1, A.H);
        }
    }
    // ---- the finish k_icf_estimate calls too, the listed entries, and the answer at every asked place of the target
    float v;
    const int32_t status = icf_estimate_finish(num, den, cnt, own != 0, A.boolean_data, v);
    if (lane < filled) {
        const size_t at = (size_t)m * A.H + lane;
        A.s_item[at] = e_id;
        A.s_sim[at] = e_sim;
        A.s_pref[at] = e_pref;
    }
    for (int32_t q = A.tfirst[m] + lane; q < A.tfirst[m + 1]; q += 64) {
        const uint32_t at = A.splace[q];
        A.p_est[at] = v;
        A.p_status[at] = status;
        A.p_cnt[at] = cnt;
        A.p_rows[at] = filled;
        A.p_target[at] = m;
    }
    if (lane == 0) {
        A.walked[m] = walked;
        if (status == FY_ESTIMATE_OK) A.user_ok[k] = 1;          // (every writer stores the same word)
    }
}

// row r of asked pair t <- entry r of its target
__global__ void k_bec_compact(int64_t total, int32_t H, const int32_t* __restrict__ p_rows, const int32_t* __restrict__ start,
                              const int32_t* __restrict__ p_target, const int32_t* __restrict__ users, const int32_t* __restrict__ s_item,
                              const float* __restrict__ s_sim, const float* __restrict__ s_pref, int32_t* __restrict__ o_user,
                              int32_t* __restrict__ o_item, float* __restrict__ o_value, int32_t* __restrict__ o_aux, float* __restrict__ o_pref) {
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
        const int32_t t = (int32_t)(x / H), r = (int32_t)(x % H);
        if (r >= p_rows[t]) continue;
        const size_t from = (size_t)p_target[t] * H + r;
        const int32_t o = start[t] + r;
        o_user[o] = users[t];
        o_item[o] = s_item[from];
        o_value[o] = s_sim[from];
        o_aux[o] = t;
        o_pref[o] = s_pref[from];
    }
}

// sums of a[0 .. n) into agg[at]
template <class T>
__global__ void k_bec_sum(int64_t n, const T* __restrict__ a, unsigned long long* __restrict__ agg, int at) {
    unsigned long long mine = 0;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) mine += (unsigned long long)a[t];
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&agg[at], mine);
}

}  // namespace

fy_result* itemcf_because_prepared(fy_itemsim_job* J, const fy_itemcf_params* prm, int64_t n_all_pairs, const int32_t* users, const int32_t* items,
                                   int location, int32_t how_many) {
    Context* ctx = J->ctx;
    const int32_t H = how_many;
    if (prm->max_prefs_per_user <= 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "maxPrefsPerUser must be > 0");
    if (how_many < 1 || how_many > FY_BECAUSE_MAX) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "howMany %d: 1 .. %d", how_many, FY_BECAUSE_MAX);
    int64_t off;
    int32_t n;
    std::unique_ptr<fy_result> Rs = icf_pairs_open(J, prm, n_all_pairs, users, items, location, 5, off, n);
    if ((int64_t)n * H > (int64_t)std::numeric_limits<int32_t>::max()) FY_FAIL(FY_ERR_UNSUPPORTED, "%d pairs x howMany %d may exceed 2^31 - 1 rows", n, H);
    hipStream_t st = ctx->stream;
    Rs->bp_n = n;
    Rs->has_itemcf_because_stats = true;
    fy_itemcf_because_stats& bs = Rs->bec;
    bs.pairs_asked = n;
    bs.pair_offset = off;
    bs.rows_stored = J->store.rows;
    Rs->d_bp_user.alloc(ctx, (size_t)n);
    Rs->d_bp_item.alloc(ctx, (size_t)n);
    Rs->d_bp_est.alloc(ctx, (size_t)n);
    Rs->d_bp_status.alloc(ctx, (size_t)n);
    Rs->d_bp_cnt.alloc(ctx, (size_t)n);
    Rs->d_bp_start.alloc(ctx, (size_t)n + 1);
    if (n == 0) {
        Rs->d_pref.alloc(ctx, 0);
        Rs->d_bp_start.zero();
        sync(ctx);
        return icfr_no_rows(std::move(Rs));
    }

    IcfrTimers tm(ctx);
    unsigned long long h_agg[BEC_AGG] = {};
    SyncOnUnwind drain(st);      // behind the host ends of the queued copies (and the caller's id arrays); the buffers below are released before it drains
    const size_t sp_total = tm.total.begin();
    size_t sp_tab = tm.tables.begin();
    DevBuf<unsigned long long> agg(ctx, BEC_AGG);
    agg.zero();
    DevBuf<int32_t> p_rows(ctx, (size_t)n + 1), p_target(ctx, (size_t)n);
    p_rows.zero();
    Rs->d_bp_cnt.zero();

    // ---- the front half (fy_itemcf_pairs.hip): known users, their rows in the store, keys, sort, targets
    IcfPairTargets T;
    icf_pair_targets(J, prm->max_prefs_per_user, n, users + off, items + off, location, Rs->d_bp_user.get(), Rs->d_bp_item.get(), Rs->d_bp_est.get(),
                     Rs->d_bp_status.get(), tm, sp_tab, T, "because");
    tm.tables.end(sp_tab);
    bs.users_known = T.n_known;
    icfr_report(bs, T.built, T.n_known > 0);
    const int32_t n_targets = T.n_targets;
    DevBuf<int32_t> s_item;
    DevBuf<float> s_sim, s_pref;
    const size_t sp_score = tm.score.begin();
    if (n_targets > 0) {
        // ---- the explanation kernel: one wave per target
        s_item.alloc(ctx, (size_t)n_targets * H);
        s_sim.alloc(ctx, (size_t)n_targets * H);
        s_pref.alloc(ctx, (size_t)n_targets * H);
        DevBuf<long long> walked(ctx, (size_t)n_targets);
        DevBuf<int32_t> user_ok(ctx, (size_t)T.n_known);
        user_ok.zero();
        BecArgs A{};
        icf_pair_args(A, J, T, prm->boolean_data);
        A.rank_item_raw = J->P.rank_item_raw.get(); A.n_targets = n_targets; A.H = H;
        A.s_item = s_item.get(); A.s_sim = s_sim.get(); A.s_pref = s_pref.get();
        A.p_est = Rs->d_bp_est.get(); A.p_status = Rs->d_bp_status.get(); A.p_cnt = Rs->d_bp_cnt.get();
        A.p_rows = p_rows.get(); A.p_target = p_target.get(); A.walked = walked.get(); A.user_ok = user_ok.get();
        k_icf_because<<<(int)ceil_div((int64_t)n_targets, (int64_t)4), 256, 0, st>>>(A);
        FY_KERNEL_CHECK();
        k_bec_sum<long long><<<grid_for(n_targets), 256, 0, st>>>(n_targets, walked.get(), agg.get(), 9);
        FY_KERNEL_CHECK();
        k_bec_sum<int32_t><<<grid_for(T.n_known), 256, 0, st>>>(T.n_known, user_ok.get(), agg.get(), 8);
        FY_KERNEL_CHECK();
        k_bec_sum<int32_t><<<grid_for(n), 256, 0, st>>>(n, Rs->d_bp_cnt.get(), agg.get(), 10);
        FY_KERNEL_CHECK();
    }
    // ---- listed rows per asked pair -> first row; the grouped rows
    exclusive_scan_i32(ctx, p_rows.get(), Rs->d_bp_start.get(), (size_t)n + 1);
    const int32_t rows = fetch(ctx, Rs->d_bp_start.get() + n);
    if (rows < 0 || (int64_t)rows > (int64_t)n * H || (n_targets == 0 && rows != 0)) FY_FAIL(FY_ERR_HIP, "because: %d rows for %d pairs x %d", rows, n, H);
    Rs->n = rows;
    Rs->d_key0.alloc(ctx, (size_t)rows);
    Rs->d_key1.alloc(ctx, (size_t)rows);
    Rs->d_value.alloc(ctx, (size_t)rows);
    Rs->d_aux.alloc(ctx, (size_t)rows);
    Rs->d_pref.alloc(ctx, (size_t)rows);
    if (rows > 0) {
        const int64_t total = (int64_t)n * H;
        k_bec_compact<<<grid_for(total), 256, 0, st>>>(total, H, p_rows.get(), Rs->d_bp_start.get(), p_target.get(), T.d_users, s_item.get(), s_sim.get(),
                                                      s_pref.get(), Rs->d_key0.get(), Rs->d_key1.get(), Rs->d_value.get(), Rs->d_aux.get(), Rs->d_pref.get());
        FY_KERNEL_CHECK();
    }
    tm.score.end(sp_score);
    icf_pairs_close(Rs.get(), n, Rs->d_bp_status.get(), agg, h_agg, bs.by_status, T.built, n_targets > 0 ? 1 : 0, tm, sp_total);
    bs.targets = n_targets;
    bs.rows = rows;
    bs.contributors = (int64_t)h_agg[10];
    bs.row_entries_walked = (int64_t)h_agg[9];
    return Rs.release();
}

}  // namespace fy
