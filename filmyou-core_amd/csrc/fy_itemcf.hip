// fy_itemcf.hip -- item-based CF recommendation on top of the similarity matrix ("next" row 1).
//
// Replaces the partialMultiply + aggregateAndRecommend jobs of M/baselinerecommender/BaselineRecommenderJob.java:285-328,
// 340-393.  Followed in the reference tree: M/baselinerecommender/BaselineAggregateAndRecommendReducer.java:97-161
// (numerators / denominators / "at least 2 datapoints"), :80-96 (boolean data), :195-235 ((float) cast, NaN skipped, top
// numRecommendations).  The Mahout 0.8 mappers in front of it are third-party and restated from the published
// algorithm (unverified, see oracle/itemcf_oracle.c): strongest maxPrefsPerUser preferences kept (ties at the cut
// kept), the column of item j = its similarity row plus (j, NaN).  PARITY UNPINNED: no reference test covers the package.
//
// Layout: users in batches; per batch dense fp64 numerator / denominator and int32 count rows in HBM (one row per
// user, columns in popularity order).  One wave per user walks the user's kept preferences in order and adds the
// similarity row of each (<= maxSimilaritiesPerRow entries, one per lane) with L2 atomics, so the per-cell order of
// additions is the order of the preferences; a second kernel turns the cells into float predictions (NaN = skip) and the
// top-N kernels of the RM2 job pick the lists.
//
// Restricted pass (fy_itemcf_recommend_filtered: usersFile / itemsFile, BaselineRecommenderJob.java:74, 189, 305-307 and
// BaselineAggregateAndRecommendReducer.java:61, 170-181, 209): the requested users are compacted into a list of slots in slot
// order and the same kernels walk batches of that LIST through one indirection (template argument LIST), so the dense rows and
// every per-user array are sized by the request; the allowed items are a bitmap over the columns that k_icf_finalize consults
// where a cell becomes a prediction (template argument ALLOW): a forbidden item is NaN before the top-N kernels see the row.
// The same pass also serves fy_ratings_shifted (ratingShift) and fy_itemsim_pairs (outputPathForSimilarityMatrix) below.
#include <algorithm>
#include <cmath>
#include <memory>

#include "fy_itemcf_request.hpp"
#include "fy_prep.hpp"
#include "fy_rm2.hpp"

namespace fy {

// similarity rows (grouped by item) -> per-column row start / length, entries re-expressed as columns
__global__ void k_icf_index_sims(int64_t n, const int32_t* __restrict__ s_item, const int32_t* __restrict__ s_other,
                                 const int32_t* __restrict__ iid, int32_t nI, const int32_t* __restrict__ pair_rank,
                                 int32_t* __restrict__ col_other, int32_t* __restrict__ row_start, int32_t* __restrict__ row_cnt) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        col_other[t] = icf_column(iid, nI, pair_rank, s_other[t]);
        const int32_t it = s_item[t];
        const int32_t row = icf_column(iid, nI, pair_rank, it);
        if (row < 0) continue;
        if (t == 0 || s_item[t - 1] != it) row_start[row] = (int32_t)t;
        atomicAdd(&row_cnt[row], 1);
    }
}

__device__ __forceinline__ uint32_t icf_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// one wave per user: threshold = the maxPrefs-th largest preference value when the user has more (else -inf):
// radix select on the order-preserving integer image, four 8-bit passes with a per-wave LDS histogram.
// Users lo .. hi: slots, or (LIST) positions of the slot list; thr is indexed by user - lo either way.
template <bool LIST>
__global__ void k_icf_threshold(int32_t lo, int32_t hi, const int32_t* __restrict__ list, const int32_t* __restrict__ rowptr,
                                const float* __restrict__ csr_r, int32_t max_prefs, float* __restrict__ thr) {
    __shared__ uint32_t hist[4][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    for (int32_t k = lo + blockIdx.x * wpb + w; k < hi; k += gridDim.x * wpb) {
        const int32_t s = LIST ? list[k] : k;
        const int32_t a = rowptr[s], b = rowptr[s + 1];
        if (b - a <= max_prefs) {
            if (lane == 0) thr[k - lo] = -INFINITY;
            continue;
        }
        uint32_t prefix = 0, mask = 0, need = (uint32_t)max_prefs;
        for (int pass = 0; pass < 4; pass++) {
            const int shift = 24 - 8 * pass;
            for (int x = lane; x < 256; x += 64) hist[w][x] = 0;
            __builtin_amdgcn_wave_barrier();
            for (int32_t f = a + lane; f < b; f += 64) {
                const uint32_t key = icf_key(csr_r[f]);
                if ((key & mask) == prefix) atomicAdd(&hist[w][(key >> shift) & 255u], 1u);
            }
            __builtin_amdgcn_wave_barrier();
            // lane 0 scans the 256 bins from the top
            uint32_t chosen = 0, cum = 0;
            if (lane == 0) {
                int x = 255;
                for (; x > 0; x--) {
                    if (cum + hist[w][x] >= need) break;
                    cum += hist[w][x];
                }
                chosen = (uint32_t)x;
            }
            chosen = __builtin_amdgcn_readfirstlane(chosen);
            cum = __builtin_amdgcn_readfirstlane(cum);
            prefix |= chosen << shift;
            mask |= 255u << shift;
            need -= cum;
            __builtin_amdgcn_wave_barrier();
        }
        if (lane == 0) {
            const uint32_t bkey = (prefix & 0x80000000u) ? (prefix & 0x7FFFFFFFu) : ~prefix;
            thr[k - lo] = __uint_as_float(bkey);
        }
    }
}

struct IcfArgs {
    const int32_t* __restrict__ rowptr;
    const int32_t* __restrict__ csr_idx;
    const float* __restrict__ csr_r;
    const float* __restrict__ thr;         // by user - slot_lo
    const int32_t* __restrict__ row_start;
    const int32_t* __restrict__ row_cnt;
    const int32_t* __restrict__ col_other;
    const float* __restrict__ sim;
    int32_t slot_lo, slot0, n_users, boolean_data;
    int64_t ld;
    double* __restrict__ num;
    double* __restrict__ den;
    int32_t* __restrict__ cnt;
    const int32_t* __restrict__ list;      // LIST: slot of user k (slot_lo / slot0 then count list positions)
};

template <bool LIST>
__global__ void k_icf_accumulate(IcfArgs A) {
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int32_t u = blockIdx.x * wpb + (threadIdx.x >> 6); u < A.n_users; u += gridDim.x * wpb) {
        const int32_t slot = LIST ? A.list[A.slot0 + u] : A.slot0 + u;
        const float thr = A.thr[A.slot0 + u - A.slot_lo];
        double* __restrict__ num = A.num + (int64_t)u * A.ld;
        double* __restrict__ den = A.den + (int64_t)u * A.ld;
        int32_t* __restrict__ cnt = A.cnt + (int64_t)u * A.ld;
        for (int32_t f = A.rowptr[slot]; f < A.rowptr[slot + 1]; f++) {   // preferences in a fixed order
            const float p = A.csr_r[f];
            if (p < thr) continue;
            const int32_t j = A.csr_idx[f];
            const int32_t n = A.row_cnt[j];
            if (n == 0) continue;                                          // no similarity row: contributes nothing
            const int32_t t0 = A.row_start[j];
            const double pd = A.boolean_data ? 1.0 : (double)p;
            for (int32_t t = t0 + lane; t < t0 + n; t += 64) {
                const int32_t i = A.col_other[t];
                if (i < 0) continue;
                const double s = (double)A.sim[t];
                atomicAdd(&num[i], pd * s);
                atomicAdd(&den[i], fabs(s));
                atomicAdd(&cnt[i], 1);
            }
            if (lane == 0) {   // the (j, NaN) entry of the wrapped similarity column: the item itself drops out
                atomicAdd(&num[j], __builtin_nan(""));
                atomicAdd(&den[j], __builtin_nan(""));
                atomicAdd(&cnt[j], 1);
            }
        }
    }
}

// cells -> float predictions (NaN = not recommendable); valid predictions counted per user.  ALLOW: only the columns whose bit is
// set in `allow` may become a prediction (itemsToRecommendFor.contains, BaselineAggregateAndRecommendReducer.java:209).
template <bool ALLOW>
__global__ void k_icf_finalize(int32_t n_users, int32_t n_cols, int64_t ld, const double* __restrict__ num,
                               const double* __restrict__ den, const int32_t* __restrict__ cnt, int32_t boolean_data,
                               int32_t top_n, const uint32_t* __restrict__ allow, float* __restrict__ S, int32_t* __restrict__ n_out) {
    const int u = blockIdx.x;
    __shared__ int sh_valid;
    if (threadIdx.x == 0) sh_valid = 0;
    __syncthreads();
    int valid = 0;
    const float qnan = __builtin_nanf("");
    for (int i = threadIdx.x; i < (int)ld; i += blockDim.x) {
        float v = qnan;
        if (i < n_cols && (!ALLOW || ((allow[i >> 5] >> (i & 31)) & 1u))) {
            const int64_t o = (int64_t)u * ld + i;
            const int32_t c = cnt[o];
            // The reducer walks numerators.nonZeroes() and recommendationVector.nonZeroes()
            // (BaselineAggregateAndRecommendReducer.java:148, 195): a cell whose numerator is exactly 0 (similarities of both
            // signs that cancel, or 0-valued preferences) never reaches the top-N queue.
            const double nm = num[o];
            if (nm != 0.0) {
                if (boolean_data) { if (c > 0) v = (float)nm; }
                else if (c > 1) v = (float)(nm / den[o]);
            }
        }
        S[(int64_t)u * ld + i] = v;
        valid += (v == v);
    }
    for (int o = 32; o > 0; o >>= 1) valid += __shfl_down(valid, o, 64);
    if ((threadIdx.x & 63) == 0 && valid) atomicAdd(&sh_valid, valid);
    __syncthreads();
    if (threadIdx.x == 0) n_out[u] = min(top_n, sh_valid);
}

__global__ void k_icf_offsets(int32_t n_users, int32_t top_n, int32_t* __restrict__ off) {
    for (int32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < n_users; u += gridDim.x * blockDim.x) off[u] = u * top_n;
}

__global__ void k_icf_compact(int32_t n_users, int32_t top_n, const int32_t* __restrict__ cnt, const int32_t* __restrict__ off,
                              const int32_t* __restrict__ p_user, const int32_t* __restrict__ p_item, const float* __restrict__ p_score,
                              int32_t* __restrict__ o_user, int32_t* __restrict__ o_item, float* __restrict__ o_score,
                              int32_t* __restrict__ o_aux) {
    const int wpb = blockDim.x >> 6, lane = threadIdx.x & 63;
    for (int32_t u = blockIdx.x * wpb + (threadIdx.x >> 6); u < n_users; u += gridDim.x * wpb)
        for (int i = lane; i < cnt[u]; i += 64) {
            const int64_t src = (int64_t)u * top_n + i, dst = (int64_t)off[u] + i;
            o_user[dst] = p_user[src];
            o_item[dst] = p_item[src];
            o_score[dst] = p_score[src];
            o_aux[dst] = 0;
        }
}

// ---------------------------------------------------------------- usersFile / itemsFile on the device
// requested raw user ids -> a flag per slot.  An id nobody has (no kept preference: UserVectorSplitterMapper never sees such a
// user) sets nothing, a duplicate sets the same flag again.
__global__ void k_icf_mark_users(int64_t n, const int32_t* __restrict__ ids, const int32_t* __restrict__ uid, int32_t nU,
                                 const int32_t* __restrict__ du2slot, int32_t* __restrict__ flag) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t du = icf_find_user(uid, nU, ids[t]);
        if (du >= 0) flag[du2slot[du]] = 1;
    }
}

// flagged slots -> the slot list, in slot order (pos = exclusive prefix of flag), and the dense user index of every entry
__global__ void k_icf_list_users(int32_t nU, const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                                 const int32_t* __restrict__ slot2du, int32_t* __restrict__ list, int32_t* __restrict__ list_du) {
    for (int32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nU; s += gridDim.x * blockDim.x)
        if (flag[s]) {
            list[pos[s]] = s;
            list_du[pos[s]] = slot2du[s];
        }
}

__global__ void k_icf_all_users(int32_t nU, const int32_t* __restrict__ slot2du, int32_t* __restrict__ list, int32_t* __restrict__ list_du) {
    for (int32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nU; s += gridDim.x * blockDim.x) {
        list[s] = s;
        list_du[s] = slot2du[s];
    }
}

// allowed raw item ids -> bitmap over the columns; an item nobody rated has no column
__global__ void k_icf_mark_items(int64_t n, const int32_t* __restrict__ ids, const int32_t* __restrict__ iid, int32_t nI,
                                 const int32_t* __restrict__ pair_rank, uint32_t* __restrict__ allow) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t col = icf_column(iid, nI, pair_rank, ids[t]);
        if (col >= 0) atomicOr(&allow[col >> 5], 1u << (col & 31));
    }
}

__global__ void k_icf_count_lists(int32_t n, const int32_t* __restrict__ n_out, int32_t* __restrict__ total) {
    int32_t mine = 0;
    for (int32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < n; u += gridDim.x * blockDim.x) mine += n_out[u] > 0;
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(total, mine);
}

// what the pass refuses before it touches the device (the request pass of fy_itemcf_request.hip refuses the same)
void icf_check_arguments(const fy_itemcf_params* prm, const fy_itemcf_filter* filt) {
    if (prm->num_recommendations <= 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "numRecommendations must be > 0");
    if (prm->num_recommendations > 2048) FY_FAIL(FY_ERR_UNSUPPORTED, "numRecommendations %d exceeds the top-N kernel limit 2048", prm->num_recommendations);
    if (prm->max_prefs_per_user <= 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "maxPrefsPerUser must be > 0");
    if (prm->world <= 0 || prm->rank < 0 || prm->rank >= prm->world) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "rank %d of world %d", prm->rank, prm->world);
    const bool by_items = filt && filt->has_items;
    if (filt && filt->has_users && (filt->n_users < 0 || (filt->n_users > 0 && !filt->users))) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "users is NULL or n_users < 0");
    if (by_items && (filt->n_items < 0 || (filt->n_items > 0 && !filt->items))) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "items is NULL or n_items < 0");
}

void icf_allow_bitmap(Context* ctx, const Prepared& P, const fy_itemcf_filter* filt, DevBuf<uint32_t>& allow) {
    hipStream_t st = ctx->stream;
    DevBuf<int32_t> ids(ctx, (size_t)filt->n_items);
    allow.alloc(ctx, (size_t)ceil_div(P.nP, 32));
    allow.zero();
    h2d(ctx, ids.get(), filt->items, (size_t)filt->n_items);
    k_icf_mark_items<<<grid_for(filt->n_items), 256, 0, st>>>(filt->n_items, ids.get(), P.iid.get(), P.nI, P.pair_rank.get(), allow.get());
    FY_KERNEL_CHECK();
}

void icf_thresholds(Context* ctx, const IcfRowView& V, const int32_t* list, int32_t lo, int32_t hi, int32_t max_prefs, float* thr) {
    if (hi <= lo) return;
    hipStream_t st = ctx->stream;
    const int g = grid_for((int64_t)(hi - lo) * 64, 256);
    if (list) k_icf_threshold<true><<<g, 256, 0, st>>>(lo, hi, list, V.rowptr, V.csr_r, max_prefs, thr);
    else k_icf_threshold<false><<<g, 256, 0, st>>>(lo, hi, nullptr, V.rowptr, V.csr_r, max_prefs, thr);
    FY_KERNEL_CHECK();
}

void icf_score_lists(Context* ctx, const fy_itemcf_params* prm, const IcfRowView& V, const IcfSims& S_, const int32_t* list, const int32_t* list_du,
                     const uint32_t* allow, int32_t lo, int32_t hi, const float* thr, fy_result* Rs, EventTimer& t_score, EventTimer& t_topn,
                     DevBuf<int32_t>& n_lists) {
    hipStream_t st = ctx->stream;
    const bool by_list = list != nullptr, by_items = allow != nullptr;
    const int32_t nI = V.n_cols, N = prm->num_recommendations, nmine = hi - lo;
    // ---- batches of users with dense accumulators
    const int64_t ld = round_up(nI, 256);
    const int64_t per_user = ld * (8 + 8 + 4 + 4);
    int64_t B = std::max<int64_t>(1, ((int64_t)8 << 30) / per_user);
    B = std::min<int64_t>(B, std::max<int32_t>(nmine, 1));
    DevBuf<double> num(ctx, (size_t)(B * ld)), den(ctx, (size_t)(B * ld));
    DevBuf<int32_t> cnt(ctx, (size_t)(B * ld));
    DevBuf<float> S(ctx, (size_t)(B * ld));
    DevBuf<int32_t> n_out(ctx, (size_t)nmine + 1), pad_off(ctx, (size_t)nmine + 1), overflow(ctx, (size_t)B), any_overflow(ctx, 1);
    DevBuf<int32_t> p_user(ctx, (size_t)nmine * N), p_item(ctx, (size_t)nmine * N);
    DevBuf<float> p_score(ctx, (size_t)nmine * N);
    DevBuf<int32_t> p_aux(ctx, (size_t)nmine * N);
    n_out.zero();
    if (nmine > 0) {
        k_icf_offsets<<<grid_for(nmine), 256, 0, st>>>(nmine, N, pad_off.get());
        FY_KERNEL_CHECK();
    }
    for (int32_t s0 = lo; s0 < hi; s0 += (int32_t)B) {
        const int32_t nb = (int32_t)std::min<int64_t>(B, hi - s0);
        const size_t sp3 = t_score.begin();
        FY_HIP(hipMemsetAsync(num.get(), 0, (size_t)nb * ld * 8, st));
        FY_HIP(hipMemsetAsync(den.get(), 0, (size_t)nb * ld * 8, st));
        FY_HIP(hipMemsetAsync(cnt.get(), 0, (size_t)nb * ld * 4, st));
        IcfArgs A{V.rowptr, V.csr_idx, V.csr_r, thr, S_.row_start, S_.row_cnt, S_.col_other,
                  S_.sim, lo, s0, nb, prm->boolean_data, ld, num.get(), den.get(), cnt.get(), list};
        const int g = grid_for((int64_t)nb * 64, 256, 256 * 32);
        if (by_list) k_icf_accumulate<true><<<g, 256, 0, st>>>(A);
        else k_icf_accumulate<false><<<g, 256, 0, st>>>(A);
        FY_KERNEL_CHECK();
        if (by_items) k_icf_finalize<true><<<nb, 256, 0, st>>>(nb, nI, ld, num.get(), den.get(), cnt.get(), prm->boolean_data, N, allow, S.get(), n_out.get() + (s0 - lo));
        else k_icf_finalize<false><<<nb, 256, 0, st>>>(nb, nI, ld, num.get(), den.get(), cnt.get(), prm->boolean_data, N, nullptr, S.get(), n_out.get() + (s0 - lo));
        FY_KERNEL_CHECK();
        t_score.end(sp3);
        const size_t sp4 = t_topn.begin();
        // (the top-N kernels name row u's user through slot2du[slot0 + u]: with a list that is the list's own dense-index column)
        launch_topn_rows(ctx, st, S.get(), ld, nI, nb, n_out.get() + (s0 - lo), pad_off.get() + (s0 - lo), V.rank_item_raw,
                         by_list ? list_du : V.slot2du, V.uid, s0, 0, p_user.get(), p_item.get(), p_score.get(), p_aux.get(),
                         overflow.get(), any_overflow.get());
        t_topn.end(sp4);
    }
    // ---- compact the padded lists
    DevBuf<int32_t> off(ctx, (size_t)nmine + 1);
    n_lists.alloc(ctx, 1);
    if (by_list) {
        n_lists.zero();
        if (nmine > 0) {
            k_icf_count_lists<<<grid_for(nmine), 256, 0, st>>>(nmine, n_out.get(), n_lists.get());
            FY_KERNEL_CHECK();
        }
    }
    exclusive_scan_i32(ctx, n_out.get(), off.get(), (size_t)nmine + 1);
    const int64_t n = nmine > 0 ? (int64_t)fetch(ctx, off.get() + nmine) : 0;
    Rs->n = n;
    Rs->d_key0.alloc(ctx, (size_t)n);
    Rs->d_key1.alloc(ctx, (size_t)n);
    Rs->d_value.alloc(ctx, (size_t)n);
    Rs->d_aux.alloc(ctx, (size_t)n);
    if (n > 0) {
        k_icf_compact<<<grid_for((int64_t)nmine * 64, 256), 256, 0, st>>>(nmine, N, n_out.get(), off.get(), p_user.get(), p_item.get(),
                                                                          p_score.get(), Rs->d_key0.get(), Rs->d_key1.get(),
                                                                          Rs->d_value.get(), Rs->d_aux.get());
        FY_KERNEL_CHECK();
    }
}

// filt == nullptr: every user of the rank's slot range, every item (fy_itemcf_recommend)
static fy_result* icf_run(Context* ctx, const fy_itemcf_params* prm, const fy_itemcf_filter* filt, const fy_ratings* R, fy_result* sims) {
    icf_check_arguments(prm, filt);
    const bool by_list = filt != nullptr, by_items = filt && filt->has_items;
    hipStream_t st = ctx->stream;
    SyncOnUnwind drain(st);   // the caller's id arrays are uploaded asynchronously
    std::unique_ptr<fy_result> Rs(new fy_result);
    Rs->ctx = ctx;
    Rs->kind = 2;
    EventTimer t_total(ctx), t_prep(ctx), t_index(ctx), t_score(ctx), t_topn(ctx);
    const size_t sp0 = t_total.begin();
    const size_t sp1 = t_prep.begin();
    Prepared P;
    build_structure(ctx, R, 1, 0, nullptr, nullptr, nullptr, true, P);
    t_prep.end(sp1);
    Rs->st.nnz = P.nnz;
    Rs->st.n_users = P.nU;
    Rs->st.n_items = P.nI;
    Rs->d_user_id.alloc(ctx, 0);
    Rs->d_item_id.alloc(ctx, 0);
    // Mahout's empty id set: nobody is asked for / nothing may be recommended
    const bool nothing = filt && ((filt->has_users && filt->n_users == 0) || (filt->has_items && filt->n_items == 0));
    if (P.nnz == 0 || nothing) {
        t_total.end(sp0);
        sync(ctx);
        Rs->st.ms_prepare = t_prep.total_ms();
        Rs->st.ms_total = t_total.total_ms();
        return Rs.release();
    }
    const int32_t nI = P.nP;
    const int64_t n_sim = sims->n;
    // ---- similarity rows by column
    const size_t sp2 = t_index.begin();
    DevBuf<int32_t> col_other(ctx, (size_t)n_sim), row_start(ctx, (size_t)nI), row_cnt(ctx, (size_t)nI);
    row_start.zero();
    row_cnt.zero();
    if (n_sim > 0) {
        k_icf_index_sims<<<grid_for(n_sim), 256, 0, st>>>(n_sim, sims->d_key0.get(), sims->d_key1.get(), P.iid.get(), P.nI,
                                                          P.pair_rank.get(), col_other.get(), row_start.get(), row_cnt.get());
        FY_KERNEL_CHECK();
    }
    // ---- the request: slot list (slot order) and column bitmap
    DevBuf<int32_t> list, list_du;
    DevBuf<uint32_t> allow;
    int32_t n_all = P.nU;
    if (by_list) {
        list.alloc(ctx, (size_t)P.nU);
        list_du.alloc(ctx, (size_t)P.nU);
        if (filt->has_users) {
            DevBuf<int32_t> ids(ctx, (size_t)filt->n_users), flag(ctx, (size_t)P.nU + 1), pos(ctx, (size_t)P.nU + 1);
            flag.zero();
            h2d(ctx, ids.get(), filt->users, (size_t)filt->n_users);
            k_icf_mark_users<<<grid_for(filt->n_users), 256, 0, st>>>(filt->n_users, ids.get(), P.uid.get(), P.nU, P.du2slot.get(), flag.get());
            FY_KERNEL_CHECK();
            exclusive_scan_i32(ctx, flag.get(), pos.get(), (size_t)P.nU + 1);
            k_icf_list_users<<<grid_for(P.nU), 256, 0, st>>>(P.nU, flag.get(), pos.get(), P.slot2du.get(), list.get(), list_du.get());
            FY_KERNEL_CHECK();
            n_all = fetch(ctx, pos.get() + P.nU);
        } else {
            k_icf_all_users<<<grid_for(P.nU), 256, 0, st>>>(P.nU, P.slot2du.get(), list.get(), list_du.get());
            FY_KERNEL_CHECK();
        }
    }
    if (by_items) icf_allow_bitmap(ctx, P, filt, allow);
    t_index.end(sp2);
    // ---- this rank's users: a contiguous range of the (degree-sorted) slot order, or of the slot list
    int32_t lo = 0, hi = n_all;
    if (prm->world > 1) {
        lo = (int32_t)((int64_t)n_all * prm->rank / prm->world);
        hi = (int32_t)((int64_t)n_all * (prm->rank + 1) / prm->world);
    }
    const int32_t nmine = hi - lo;
    DevBuf<float> thr(ctx, (size_t)nmine + 1);
    const IcfRowView V = icf_rows_of(P);
    icf_thresholds(ctx, V, by_list ? list.get() : nullptr, lo, hi, prm->max_prefs_per_user, thr.get());
    DevBuf<int32_t> n_lists;
    const IcfSims S_{row_start.get(), row_cnt.get(), col_other.get(), sims->d_value.get()};
    icf_score_lists(ctx, prm, V, S_, by_list ? list.get() : nullptr, by_list ? list_du.get() : nullptr, by_items ? allow.get() : nullptr, lo, hi,
                    thr.get(), Rs.get(), t_score, t_topn, n_lists);
    const int64_t n = Rs->n;
    t_total.end(sp0);
    // the unrestricted job reports the users it walked; the restricted one the users that received a list
    const int64_t scored = by_list ? (int64_t)fetch(ctx, n_lists.get()) : nmine;
    sync(ctx);
    Rs->st.recs = n;
    Rs->st.users_scored = scored;
    Rs->st.ms_prepare = t_prep.total_ms();
    Rs->st.ms_total = t_total.total_ms();
    if (by_list) {   // per phase: similarity rows re-indexed + the request's list and bitmap, accumulate + finalize, top-N
        Rs->st.ms_tables = t_index.total_ms();
        Rs->st.ms_score = t_score.total_ms();
        Rs->st.ms_topn = t_topn.total_ms();
        Rs->st.score_launches = (int64_t)t_score.count();
    }
    return Rs.release();
}

fy_result* itemcf_recommend(Context* ctx, const fy_itemcf_params* prm, const fy_ratings* R, fy_result* sims) {
    return icf_run(ctx, prm, nullptr, R, sims);
}

fy_result* itemcf_recommend_filtered(Context* ctx, const fy_itemcf_params* prm, const fy_itemcf_filter* filt, const fy_ratings* R,
                                     fy_result* sims) {
    return icf_run(ctx, prm, filt->has_users || filt->has_items ? filt : nullptr, R, sims);
}

// ---------------------------------------------------------------- ratingShift
// float prefValue = score + ratingShift (BaselineToItemPrefsMapper.java:60, BaselinePreparePreferenceMatrixJob.java:223): fp32
__global__ void k_shift_scores(int64_t n, const float* __restrict__ in, float shift, float* __restrict__ out) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) out[t] = in[t] + shift;
}

fy_ratings* ratings_shifted(Context* ctx, const fy_ratings* R, float shift) {
    std::unique_ptr<fy_ratings> r(new fy_ratings);
    const size_t n = (size_t)R->nnz;
    r->ctx = ctx;
    r->nnz = R->nnz;
    r->user.alloc(ctx, n);
    r->item.alloc(ctx, n);
    r->score.alloc(ctx, n);
    if (n) {
        d2d(ctx, r->user.get(), R->user.get(), n);
        d2d(ctx, r->item.get(), R->item.get(), n);
        k_shift_scores<<<grid_for(R->nnz), 256, 0, ctx->stream>>>(R->nnz, R->score.get(), shift, r->score.get());
        FY_KERNEL_CHECK();
        ratings_id_bounds(ctx, r.get());   // ids as before; whether the shifted scores are still fp16-exact is found again
    }
    return r.release();
}

// ---------------------------------------------------------------- similarity matrix as item pairs
// Mahout 0.8's ItemSimilarityJob.MostSimilarItemPairsMapper / Reducer (third-party, restated from memory like every Mahout class of
// this package: PARITY UNPINNED) write each entry of the similarity rows once per unordered pair.  Here: the ordered entries
// (item, other) are sorted; an entry with item < other stands for its pair, one with item > other only when (other, item) is not
// among the entries -- row `other` is searched in the sorted keys --, and the survivors are sorted by (min, max).
__global__ void k_pairs_keys(int64_t n, const int32_t* __restrict__ item, const int32_t* __restrict__ other, uint64_t* __restrict__ keys) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        keys[t] = ((uint64_t)(uint32_t)item[t] << 32) | (uint32_t)other[t];
}

__global__ void k_pairs_select(int64_t n, const int32_t* __restrict__ item, const int32_t* __restrict__ other,
                               const uint64_t* __restrict__ sorted, uint64_t* __restrict__ keys, unsigned long long* __restrict__ kept) {
    int mine = 0;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t i = (uint32_t)item[t], j = (uint32_t)other[t];
        bool keep = i <= j;
        if (!keep) {
            const uint64_t want = ((uint64_t)j << 32) | i;
            int64_t lo = 0, hi = n;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (sorted[mid] < want) lo = mid + 1; else hi = mid;
            }
            keep = !(lo < n && sorted[lo] == want);
        }
        keys[t] = keep ? (((uint64_t)(i < j ? i : j) << 32) | (i < j ? j : i)) : ~0ull;   // dropped entries sort behind every pair
        mine += keep;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(kept, (unsigned long long)mine);
}

__global__ void k_pairs_emit(int64_t n, const uint64_t* __restrict__ keys, int32_t* __restrict__ a, int32_t* __restrict__ b, int32_t* __restrict__ aux) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        a[t] = (int32_t)(keys[t] >> 32);
        b[t] = (int32_t)(uint32_t)keys[t];
        aux[t] = 0;
    }
}

fy_result* itemsim_pairs(Context* ctx, fy_result* sims) {
    hipStream_t st = ctx->stream;
    std::unique_ptr<fy_result> Rs(new fy_result);
    Rs->ctx = ctx;
    Rs->kind = 3;
    Rs->d_user_id.alloc(ctx, 0);
    Rs->d_item_id.alloc(ctx, 0);
    EventTimer t_total(ctx);
    const size_t sp0 = t_total.begin();
    const int64_t n = sims->n;
    int64_t kept = 0;
    DevBuf<uint64_t> k0(ctx, (size_t)n), k1(ctx, (size_t)n), k2(ctx, (size_t)n);
    DevBuf<float> v(ctx, (size_t)n);
    if (n > 0) {
        DevBuf<unsigned long long> d_kept(ctx, 1);
        d_kept.zero();
        k_pairs_keys<<<grid_for(n), 256, 0, st>>>(n, sims->d_key0.get(), sims->d_key1.get(), k0.get());
        FY_KERNEL_CHECK();
        sort_keys_u64(ctx, k0.get(), k1.get(), (size_t)n);
        k_pairs_select<<<grid_for(n), 256, 0, st>>>(n, sims->d_key0.get(), sims->d_key1.get(), k1.get(), k0.get(), d_kept.get());
        FY_KERNEL_CHECK();
        sort_pairs_u64_f32(ctx, k0.get(), k2.get(), sims->d_value.get(), v.get(), (size_t)n);   // (inputs are only read)
        kept = (int64_t)fetch(ctx, d_kept.get());
    }
    Rs->n = kept;
    Rs->d_key0.alloc(ctx, (size_t)kept);
    Rs->d_key1.alloc(ctx, (size_t)kept);
    Rs->d_value.alloc(ctx, (size_t)kept);
    Rs->d_aux.alloc(ctx, (size_t)kept);
    if (kept > 0) {
        k_pairs_emit<<<grid_for(kept), 256, 0, st>>>(kept, k2.get(), Rs->d_key0.get(), Rs->d_key1.get(), Rs->d_aux.get());
        FY_KERNEL_CHECK();
        d2d(ctx, Rs->d_value.get(), v.get(), (size_t)kept);
    }
    t_total.end(sp0);
    sync(ctx);
    Rs->st.n_items = sims->st.n_items;
    Rs->st.recs = kept;
    Rs->st.ms_total = t_total.total_ms();
    return Rs.release();
}

}  // namespace fy
