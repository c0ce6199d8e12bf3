// fy_itemcf_profiles.hip -- item-based lists for GIVEN profiles on a prepared similarity job (fy_itemcf_recommend_profiles).
//
// DESIGN.md section 2i.  The list pass of fy_itemcf_request.hip reads a user's preferences through an IcfRowView; here the view is a
// small CSR composed from the caller's profiles instead of the job's own CSR, and everything behind it -- thresholds, the set J, the
// row store, accumulate, finalize, top-N, the result and its statistics -- is that pass unchanged (the icfr_* frame of fy_itemcf_request.hip).  The ingest is sized by the request: T = the entries of this
// rank's profiles + (FY_PROFILE_ON_RESIDENT) the resident rows of the users they name.
//   k_prof_residents   label -> slot by icf_find_user (the search of k_icfr_find_users), the length of the resident row; scan -> roff
//   k_prof_keys        key = profile << cb | column over the T elements, resident entries IN FRONT of the profile's own entries (raw
//                      item -> column by icf_column; an entry without a column gets the key of profile n: it sorts behind everything)
//   sort_pairs_u64_u32 stable, cb + bits(n) key bits: a run of one key keeps resident-then-given order, its last element counts
//   k_prof_runs        keep = last of its run and no delete; the counters (superseded, deletes that hit / missed the resident row)
//   exclusive_scan_i32 place of every kept element = the composed CSR's entry (sorted by profile, then ascending column)
//   k_prof_rowptr      rowptr[p] = place of the first element whose key is >= p << cb (fy_lower_bound); empty profiles counted
//   k_prof_scatter     column and preference (the resident row's float or the given one, bit for bit) to their place
// All stores are plain vector stores; the counters are a handful of wave-aggregated atomics.
#include <algorithm>
#include <limits>

#include "fy_itemcf_profiles.hpp"

namespace fy {
namespace {

enum { PC_USERS_UNKNOWN = 0, PC_UNKNOWN_ITEM, PC_SUPERSEDED, PC_REMOVES_HIT, PC_REMOVES_MISSED, PC_EMPTY, PC_N };

inline int bits_for(int64_t v) {      // bits needed to hold the values 0 .. v
    int b = 1;
    while (b < 63 && (v >> b) != 0) b++;
    return b;
}

// the p in [0, n) with off[p] <= t < off[p + 1] (off ascending from 0, t < off[n])
__device__ __forceinline__ int32_t prof_owner(const int32_t* __restrict__ off, int32_t n, int32_t t) {
    return fy_lower_bound<true>(off, 0, n, t) - 1;
}

__device__ __forceinline__ void prof_count(unsigned long long* __restrict__ counters, int which, bool mine) {      // whole waves call it
    const unsigned long long b = __ballot(mine);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&counters[which], (unsigned long long)__popcll(b));
}

// slot[p] = the slot of the resident user labels[p] (-1: the job does not know the id), rlen[p] = the length of its row; rlen[n] = 0
__global__ void k_prof_residents(int32_t n, const int32_t* __restrict__ labels, const int32_t* __restrict__ uid, int32_t nU,
                                 const int32_t* __restrict__ du2slot, const int32_t* __restrict__ rowptr, int32_t* __restrict__ slot,
                                 int32_t* __restrict__ rlen, unsigned long long* __restrict__ counters) {
    const int64_t n_up = ((int64_t)n + 1 + 63) & ~(int64_t)63;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n_up; p += (int64_t)gridDim.x * blockDim.x) {
        bool unknown = false;
        if (p < n) {
            const int32_t du = icf_find_user(uid, nU, labels[p]);
            const int32_t s = du >= 0 ? du2slot[du] : -1;
            slot[p] = s;
            rlen[p] = s >= 0 ? rowptr[s + 1] - rowptr[s] : 0;
            unknown = s < 0;
        } else if (p == n) {
            rlen[p] = 0;
        }
        prof_count(counters, PC_USERS_UNKNOWN, unknown);
    }
}

struct ProfIn {
    int32_t n;                      // profiles of this rank
    int32_t T, Rn;                  // elements, of which the first Rn are resident entries
    int cb;                         // bits of a column
    const int32_t* roff;            // n + 1: first resident element of every profile (Rn > 0)
    const int32_t* slot;            // n (FY_PROFILE_ON_RESIDENT; else nullptr)
    const int32_t* start;           // n + 1: first given entry of every profile, from 0
    const int32_t* item;            // T - Rn given entries
    const float* score;
    const uint8_t* remove;          // or nullptr
    const int32_t* rowptr;          // the job's CSR
    const int32_t* csr_idx;
    const float* csr_r;
};

__global__ void k_prof_keys(ProfIn A, const int32_t* __restrict__ iid, int32_t nI, const int32_t* __restrict__ pair_rank, uint64_t* __restrict__ keys,
                            uint32_t* __restrict__ pos, unsigned long long* __restrict__ counters) {
    const int64_t t_up = ((int64_t)A.T + 63) & ~(int64_t)63;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < t_up; t += (int64_t)gridDim.x * blockDim.x) {
        bool no_column = false;
        if (t < A.T) {
            int32_t p, col;
            if (t < A.Rn) {
                p = prof_owner(A.roff, A.n, (int32_t)t);
                col = A.csr_idx[A.rowptr[A.slot[p]] + ((int32_t)t - A.roff[p])];
            } else {
                const int32_t e = (int32_t)t - A.Rn;
                p = prof_owner(A.start, A.n, e);
                col = icf_column(iid, nI, pair_rank, A.item[e]);
                no_column = col < 0;
            }
            keys[t] = no_column ? ((uint64_t)(uint32_t)A.n << A.cb) : (((uint64_t)(uint32_t)p << A.cb) | (uint32_t)col);
            pos[t] = (uint32_t)t;
        }
        prof_count(counters, PC_UNKNOWN_ITEM, no_column);
    }
}

// keep[x] (x <= T; keep[T] = 0): sorted element x is the last of its key's run, belongs to a profile and is no delete
__global__ void k_prof_runs(ProfIn A, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ spos, int32_t* __restrict__ keep,
                            unsigned long long* __restrict__ counters) {
    const int64_t t_up = ((int64_t)A.T + 1 + 63) & ~(int64_t)63;
    const uint64_t col_mask = ((uint64_t)1 << A.cb) - 1;
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < t_up; x += (int64_t)gridDim.x * blockDim.x) {
        int kind = -1;      // 0 superseded, 1 a delete that hit the resident row, 2 a delete that missed
        bool k = false;
        if (x < A.T) {
            const uint64_t key = skeys[x];
            const int32_t p = (int32_t)(key >> A.cb);
            if (p < A.n) {
                const bool last = x == A.T - 1 || skeys[x + 1] != key;
                const int32_t t = (int32_t)spos[x];
                const bool given = t >= A.Rn;
                if (!last) {
                    if (given) kind = 0;
                } else if (given && A.remove && A.remove[t - A.Rn]) {
                    bool hit = false;
                    const int32_t s = A.slot ? A.slot[p] : -1;
                    if (s >= 0) {      // is the column in the resident row (ascending columns)?
                        const int32_t col = (int32_t)(key & col_mask);
                        const int32_t end = A.rowptr[s + 1], lo = fy_lower_bound(A.csr_idx, A.rowptr[s], end, col);
                        hit = lo < end && A.csr_idx[lo] == col;
                    }
                    kind = hit ? 1 : 2;
                } else {
                    k = true;
                }
            }
        }
        if (x <= A.T) keep[x] = k;
        prof_count(counters, PC_SUPERSEDED, kind == 0);
        prof_count(counters, PC_REMOVES_HIT, kind == 1);
        prof_count(counters, PC_REMOVES_MISSED, kind == 2);
    }
}

// rowptr[p], p <= n: the place of the first kept element of profile p (place[T] = all kept elements)
__global__ void k_prof_rowptr(int32_t n, int32_t T, int cb, const uint64_t* __restrict__ skeys, const int32_t* __restrict__ place,
                              int32_t* __restrict__ rowptr, unsigned long long* __restrict__ counters) {
    const int64_t n_up = ((int64_t)n + 1 + 63) & ~(int64_t)63;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n_up; p += (int64_t)gridDim.x * blockDim.x) {
        bool empty = false;
        if (p <= n) {
            const int32_t a = place[fy_lower_bound(skeys, 0, T, (uint64_t)p << cb)];
            rowptr[p] = a;
            if (p < n) empty = place[fy_lower_bound(skeys, 0, T, (uint64_t)(p + 1) << cb)] == a;
        }
        prof_count(counters, PC_EMPTY, empty);
    }
}

__global__ void k_prof_scatter(ProfIn A, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ spos, const int32_t* __restrict__ keep,
                               const int32_t* __restrict__ place, int32_t* __restrict__ o_idx, float* __restrict__ o_r) {
    const uint64_t col_mask = ((uint64_t)1 << A.cb) - 1;
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < A.T; x += (int64_t)gridDim.x * blockDim.x) {
        if (!keep[x]) continue;
        const uint64_t key = skeys[x];
        const int32_t t = (int32_t)spos[x], at = place[x];
        float r;
        if (t < A.Rn) {
            const int32_t p = (int32_t)(key >> A.cb);
            r = A.csr_r[A.rowptr[A.slot[p]] + (t - A.roff[p])];
        } else {
            r = A.score[t - A.Rn];
        }
        o_idx[at] = (int32_t)(key & col_mask);
        o_r[at] = r;
    }
}

__global__ void k_prof_identity(int32_t n, int32_t* __restrict__ list) {
    for (int32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) list[k] = k;
}

}  // namespace

fy_result* itemcf_recommend_profiles(fy_itemsim_job* J, const fy_itemcf_params* prm, const fy_itemcf_profiles* pf, const fy_itemcf_filter* filt) {
    Context* ctx = J->ctx;
    const Prepared& P = J->P;
    // ---- what the host refuses before any launch: the list pass's own failures first
    icf_check_arguments(prm, filt);
    icfr_check_job(J);
    if (filt && filt->has_users) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "fy_itemcf_recommend_profiles takes an items-only filter (has_users must be 0): the profiles are the users");
    if (pf->n_profiles < 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "n_profiles < 0");
    if (pf->base != FY_PROFILE_WHOLE && pf->base != FY_PROFILE_ON_RESIDENT) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "base %d is neither FY_PROFILE_WHOLE nor FY_PROFILE_ON_RESIDENT", pf->base);
    const int64_t n_all = pf->n_profiles;
    if (n_all > 0 && (!pf->user || !pf->start)) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "user or start is NULL");
    if (n_all > 0) {
        if (pf->start[0] != 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "start[0] is %lld: the offsets begin at 0", (long long)pf->start[0]);
        for (int64_t p = 0; p < n_all; p++)
            if (pf->start[p + 1] < pf->start[p]) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "start decreases at profile %lld", (long long)p);
        if (pf->start[n_all] > 0 && (!pf->item || !pf->score)) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "item or score is NULL");
        if (pf->start[n_all] > (int64_t)std::numeric_limits<int32_t>::max())
            FY_FAIL(FY_ERR_UNSUPPORTED, "%lld profile entries: at most 2^31 - 1", (long long)pf->start[n_all]);
    }
    if (n_all > (int64_t)std::numeric_limits<int32_t>::max()) FY_FAIL(FY_ERR_UNSUPPORTED, "%lld profiles: at most 2^31 - 1", (long long)n_all);

    const bool by_items = filt && filt->has_items;
    hipStream_t st = ctx->stream;
    std::unique_ptr<fy_result> Rs = icfr_new_result(J, 2);
    Rs->has_itemcf_profile_stats = true;
    fy_itemcf_profile_stats& ps = Rs->cpf;
    ps.profiles_asked = n_all;
    ps.rows_stored = J->store.rows;
    if (P.nnz == 0 || n_all == 0 || (by_items && filt->n_items == 0)) return icfr_no_rows(std::move(Rs));
    icfr_check_store(J);

    // ---- this rank's profiles: a contiguous range of the list given
    int64_t plo = 0, phi = n_all;
    if (prm->world > 1) {
        plo = n_all * prm->rank / prm->world;
        phi = n_all * (prm->rank + 1) / prm->world;
    }
    const int32_t n = (int32_t)(phi - plo);
    const int64_t e0 = pf->start[plo];
    const int32_t E = (int32_t)(pf->start[phi] - e0);
    ps.profiles_mine = n;
    ps.entries = E;
    if (n == 0) return icfr_no_rows(std::move(Rs));
    const bool resident = pf->base == FY_PROFILE_ON_RESIDENT;

    IcfrTimers tm(ctx);
    std::vector<int32_t> h_start((size_t)n + 1);
    for (int32_t p = 0; p <= n; p++) h_start[(size_t)p] = (int32_t)(pf->start[plo + p] - e0);
    unsigned long long h_c[PC_N] = {};
    int32_t h_composed = 0;
    SyncOnUnwind drain(st);      // behind the host ends of the queued copies (and the caller's arrays); the buffers below are released first
    const size_t sp_total = tm.total.begin();
    const size_t sp_tab = tm.tables.begin();

    // ---- the profiles in HBM
    DevBuf<int32_t> labels(ctx, (size_t)n), start(ctx, (size_t)n + 1), item(ctx, (size_t)E);
    DevBuf<float> score(ctx, (size_t)E);
    DevBuf<uint8_t> remove;
    DevBuf<unsigned long long> counters(ctx, PC_N);
    counters.zero();
    h2d(ctx, labels.get(), pf->user + plo, (size_t)n);
    h2d(ctx, start.get(), h_start.data(), (size_t)n + 1);
    h2d(ctx, item.get(), pf->item + e0, (size_t)E);
    h2d(ctx, score.get(), pf->score + e0, (size_t)E);
    if (pf->remove && E > 0) {
        remove.alloc(ctx, (size_t)E);
        h2d(ctx, remove.get(), pf->remove + e0, (size_t)E);
    }
    // ---- FY_PROFILE_ON_RESIDENT: the named users' slots and rows
    DevBuf<int32_t> slot, rlen, roff;
    int64_t Rn = 0;
    if (resident) {
        slot.alloc(ctx, (size_t)n);
        rlen.alloc(ctx, (size_t)n + 1);
        roff.alloc(ctx, (size_t)n + 1);
        k_prof_residents<<<grid_for((int64_t)n + 1), 256, 0, st>>>(n, labels.get(), P.uid.get(), P.nU, P.du2slot.get(), P.rowptr.get(), slot.get(), rlen.get(),
                                                                   counters.get());
        FY_KERNEL_CHECK();
        exclusive_scan_i32(ctx, rlen.get(), roff.get(), (size_t)n + 1);
        if ((int64_t)n * P.nP <= (int64_t)std::numeric_limits<int32_t>::max()) {
            Rn = (int64_t)fetch(ctx, roff.get() + n);
        } else {      // the int32 prefix may have wrapped (a row holds at most nP preferences): the lengths are summed on the host
            std::vector<int32_t> h_len((size_t)n);
            d2h(ctx, h_len.data(), rlen.get(), (size_t)n);
            sync(ctx);
            for (int32_t v : h_len) Rn += v;
        }
    }
    if (Rn + E > (int64_t)std::numeric_limits<int32_t>::max())
        FY_FAIL(FY_ERR_UNSUPPORTED, "%lld resident preferences + %lld entries: a request composes at most 2^31 - 1 preferences", (long long)Rn, (long long)E);
    const int32_t T = (int32_t)(Rn + E);

    // ---- compose: keys, stable sort, last of every run, scan, scatter
    DevBuf<int32_t> c_rowptr(ctx, (size_t)n + 1), c_idx(ctx, (size_t)T), list(ctx, (size_t)n);
    DevBuf<float> c_r(ctx, (size_t)T);
    if (T > 0) {
        ProfIn A{};
        A.n = n; A.T = T; A.Rn = (int32_t)Rn;
        A.cb = bits_for((int64_t)P.nP - 1);
        A.roff = resident ? roff.get() : nullptr;
        A.slot = resident ? slot.get() : nullptr;
        A.start = start.get();
        A.item = item.get(); A.score = score.get(); A.remove = remove.get();
        A.rowptr = P.rowptr.get(); A.csr_idx = P.csr_idx.get(); A.csr_r = P.csr_r.get();
        DevBuf<uint64_t> keys(ctx, (size_t)T), skeys(ctx, (size_t)T);
        DevBuf<uint32_t> pos(ctx, (size_t)T), spos(ctx, (size_t)T);
        DevBuf<int32_t> keep(ctx, (size_t)T + 1), place(ctx, (size_t)T + 1);
        k_prof_keys<<<grid_for(T), 256, 0, st>>>(A, P.iid.get(), P.nI, P.pair_rank.get(), keys.get(), pos.get(), counters.get());
        FY_KERNEL_CHECK();
        sort_pairs_u64_u32(ctx, keys.get(), skeys.get(), pos.get(), spos.get(), (size_t)T, A.cb + bits_for(n));      // stable
        k_prof_runs<<<grid_for((int64_t)T + 1), 256, 0, st>>>(A, skeys.get(), spos.get(), keep.get(), counters.get());
        FY_KERNEL_CHECK();
        exclusive_scan_i32(ctx, keep.get(), place.get(), (size_t)T + 1);
        k_prof_rowptr<<<grid_for((int64_t)n + 1), 256, 0, st>>>(n, T, A.cb, skeys.get(), place.get(), c_rowptr.get(), counters.get());
        FY_KERNEL_CHECK();
        k_prof_scatter<<<grid_for(T), 256, 0, st>>>(A, skeys.get(), spos.get(), keep.get(), place.get(), c_idx.get(), c_r.get());
        FY_KERNEL_CHECK();
        d2h(ctx, &h_composed, place.get() + T, 1);
    }
    d2h(ctx, h_c, counters.get(), PC_N);
    sync(ctx);
    if (h_composed < 0 || h_composed > T) FY_FAIL(FY_ERR_HIP, "profiles: %d composed preferences of %d elements", h_composed, T);
    ps.users_unknown = (int64_t)h_c[PC_USERS_UNKNOWN];
    ps.entries_unknown_item = (int64_t)h_c[PC_UNKNOWN_ITEM];
    ps.entries_superseded = (int64_t)h_c[PC_SUPERSEDED];
    ps.removes_hit = (int64_t)h_c[PC_REMOVES_HIT];
    ps.removes_missed = (int64_t)h_c[PC_REMOVES_MISSED];
    ps.profiles_empty = T > 0 ? (int64_t)h_c[PC_EMPTY] : n;
    ps.prefs_composed = h_composed;
    if (h_composed == 0) return icfr_nobody(std::move(Rs), tm, sp_tab, sp_total);      // every profile is empty: nothing is built, nobody gets a list
    k_prof_identity<<<grid_for(n), 256, 0, st>>>(n, list.get());
    FY_KERNEL_CHECK();
    DevBuf<uint32_t> allow;
    if (by_items) icf_allow_bitmap(ctx, P, filt, allow);

    // ---- the list pass over the composed rows: row k of the view is profile k, named labels[k]
    const IcfRowView V{c_rowptr.get(), c_idx.get(), c_r.get(), labels.get(), list.get(), P.rank_item_raw.get(), P.nP};
    DevBuf<float> thr(ctx, (size_t)n + 1);
    IcfrRows built;
    icfr_rows_for_users(J, V, list.get(), 0, n, prm->max_prefs_per_user, thr.get(), tm, sp_tab, built);
    icfr_report(ps, built, true);
    ps.profiles_scored = icfr_lists_from_store(J, prm, V, list.get(), list.get(), by_items ? allow.get() : nullptr, 0, n, thr.get(), built, Rs.get(), tm, sp_total);
    return Rs.release();
}

}  // namespace fy
