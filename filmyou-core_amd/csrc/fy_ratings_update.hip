// fy_ratings_update.hip -- fy_ratings_apply: the ratings table's write semantics (a write to an existing (user, item) replaces the row,
// a DELETE removes it; ratings(user int, item int, score float, PRIMARY KEY (user, item))) applied to the COO in HBM.
//
//   batch  : key = (uint64) user << 32 | (uint32) item with the write's position; a stable radix sort by key leaves every run of one
//            key in batch order, its last entry is the write that counts.  The run ends form the TABLE: the distinct keys, ascending,
//            each with the position of its last write.  A 256 Ki-bit bitmap of the batch's users (bit = low 18 bits of the id: exact
//            for ids below 262 144, a one-hash filter beyond -- never a false "no") is built in the same pass.
//   source : ONE decision per entry -- user bit set?  then: key in the table? -- made twice by the same device function: the counting
//            pass reads the users (4 B per entry, items only behind a set bit) and flags the table keys it meets, the writing pass reads
//            12 B and writes 12 B per survivor.  Every wave owns a contiguous range of the source, so order is kept by a scan of two
//            levels: ballot + popcount inside the wave, an exclusive scan over the waves' survivor counts across waves and workgroups.
//            The source is never sorted.  Bitmap and table are staged in LDS once per workgroup (persistent grid: two workgroups per
//            CU); a table of more than Tuning::upd_lds_keys keys stays in global memory (L2) and is searched there.
//   append : the last writes that are not deletes, in batch order: a flag per batch position, its prefix sum is the place.
//   bounds : max ids and "every score is fp16-exact" (what fy::ratings_id_bounds finds) ride on the writing pass and the append.
#include <hip/hip_fp16.h>

#include "fy_prep.hpp"
#include "fy_ratings_update.hpp"

namespace fy {

namespace {

constexpr int UPD_BLOCK = 1024;                  // 16 waves; with 64 KiB of LDS two workgroups share a CU
constexpr int UPD_WAVES = UPD_BLOCK / 64;
constexpr int UPD_TILE = 256;                    // entries a wave takes per round (4 per lane, all loads issued before the first use)
constexpr int UPD_BITMAP_BITS = 1 << 18;
constexpr int UPD_BITMAP_WORDS = UPD_BITMAP_BITS / 32;

inline int small_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, 256), 4096)); }

__device__ __forceinline__ uint64_t upd_key(int32_t u, int32_t i) { return ((uint64_t)(uint32_t)u << 32) | (uint32_t)i; }
__device__ __forceinline__ bool upd_user_bit(const uint32_t* bitmap, int32_t u) {
    const uint32_t b = (uint32_t)u & (UPD_BITMAP_BITS - 1);
    return (bitmap[b >> 5] >> (b & 31)) & 1u;
}
// index of `want` among the m ascending distinct keys, -1 when it is not there
__device__ __forceinline__ int32_t upd_find(const uint64_t* tab, int32_t m, uint64_t want) {
    int32_t lo = 0, hi = m;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (tab[mid] < want) lo = mid + 1; else hi = mid;
    }
    return (lo < m && tab[lo] == want) ? lo : -1;
}

__global__ void k_upd_pack(int32_t n, const int32_t* __restrict__ user, const int32_t* __restrict__ item, uint64_t* __restrict__ keys,
                           uint32_t* __restrict__ pos, uint32_t* __restrict__ bitmap) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        const int32_t u = user[t];
        keys[t] = upd_key(u, item[t]);
        pos[t] = (uint32_t)t;
        const uint32_t b = (uint32_t)u & (UPD_BITMAP_BITS - 1);
        atomicOr(&bitmap[b >> 5], 1u << (b & 31));
    }
}

// is_last[t]: sorted entry t ends the run of its key; live_at[p]: the write at batch position p is the last of its key and no delete
__global__ void k_upd_runs(int32_t n, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ spos, const uint8_t* __restrict__ remove,
                           uint32_t* __restrict__ is_last, uint32_t* __restrict__ live_at) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        const bool last = t == n - 1 || skeys[t + 1] != skeys[t];
        const uint32_t p = spos[t];
        is_last[t] = last;
        live_at[p] = last && !(remove && remove[p]);
    }
}

__global__ void k_upd_table(int32_t n, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ spos, const uint32_t* __restrict__ is_last,
                            const uint32_t* __restrict__ run_incl, uint64_t* __restrict__ tkeys, uint32_t* __restrict__ tpos) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x)
        if (is_last[t]) {
            const uint32_t j = run_incl[t] - 1;
            tkeys[j] = skeys[t];
            tpos[j] = spos[t];
        }
}

struct UpdSource {
    int64_t nnz, per;               // entries, entries per wave (a multiple of UPD_TILE)
    const int32_t* user;
    const int32_t* item;
    const float* score;
    const uint32_t* bitmap;         // UPD_BITMAP_WORDS words
    const uint64_t* tkeys;          // m ascending distinct keys
    int32_t m, lds_keys;            // lds_keys = m: the table is staged in LDS; 0: it is searched in global memory
};

// WRITE = false: wave_count[w] = survivors of wave w's range, matched[j] = 1 for every table key some source entry holds.
// WRITE = true : the survivors go to out_* from wave_incl[w - 1] on, in source order; bounds[0..2] as k_max_ids leaves them.
template <bool WRITE>
__global__ void __launch_bounds__(UPD_BLOCK) k_upd_source(UpdSource S, uint32_t* __restrict__ matched, int64_t* __restrict__ wave_count,
                                                          const int64_t* __restrict__ wave_incl, int32_t* __restrict__ out_user,
                                                          int32_t* __restrict__ out_item, float* __restrict__ out_score, int32_t* __restrict__ bounds) {
    extern __shared__ uint64_t upd_lds[];                       // [lds_keys keys][UPD_BITMAP_WORDS words]
    uint64_t* lds_tab = upd_lds;
    uint32_t* lds_bits = reinterpret_cast<uint32_t*>(upd_lds + S.lds_keys);
    for (int k = threadIdx.x; k < UPD_BITMAP_WORDS; k += UPD_BLOCK) lds_bits[k] = S.bitmap[k];
    for (int k = threadIdx.x; k < S.lds_keys; k += UPD_BLOCK) lds_tab[k] = S.tkeys[k];
    __syncthreads();
    const uint64_t* tab = S.lds_keys ? lds_tab : S.tkeys;

    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * UPD_WAVES + (threadIdx.x >> 6);
    const int64_t lo = w * S.per < S.nnz ? w * S.per : S.nnz, hi = lo + S.per < S.nnz ? lo + S.per : S.nnz;
    int64_t off = 0;                                            // WRITE: next free place of this wave; else: its survivors so far
    if (WRITE) off = w ? wave_incl[w - 1] : 0;
    int32_t mu = -1, mi = -1;
    bool not_half = false;
    for (int64_t base = lo; base < hi; base += UPD_TILE) {      // wave-uniform trip count: every lane enters every ballot
        int32_t u[4], it[4];
        float s[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t t = base + k * 64 + lane;
            u[k] = t < hi ? S.user[t] : 0;
            if (WRITE) {
                it[k] = t < hi ? S.item[t] : 0;
                s[k] = t < hi ? S.score[t] : 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t t = base + k * 64 + lane;
            bool keep = t < hi;
            if (keep && upd_user_bit(lds_bits, u[k])) {
                const int32_t i = WRITE ? it[k] : S.item[t];
                const int32_t j = upd_find(tab, S.m, upd_key(u[k], i));
                if (j >= 0) {
                    keep = false;
                    if (!WRITE) matched[j] = 1u;                // every writer stores the same word
                }
            }
            const unsigned long long kept = __ballot(keep);
            if (WRITE && keep) {
                const int64_t at = off + __popcll(kept & ((1ull << lane) - 1ull));
                out_user[at] = u[k];
                out_item[at] = it[k];
                out_score[at] = s[k];
                mu = max(mu, u[k]);
                mi = max(mi, it[k]);
                if (s[k] == s[k] && __half2float(__float2half(s[k])) != s[k]) not_half = true;
            }
            off += __popcll(kept);
        }
    }
    if (!WRITE) {
        if (lane == 0) wave_count[w] = off;
        return;
    }
    if (__ballot(not_half) && lane == 0) bounds[2] = 1;
    for (int o = 32; o > 0; o >>= 1) {
        mu = max(mu, __shfl_down(mu, o, 64));
        mi = max(mi, __shfl_down(mi, o, 64));
    }
    __shared__ int32_t sh[2][UPD_WAVES];                        // one pair of atomics per workgroup, as k_max_ids
    if (lane == 0) { sh[0][threadIdx.x >> 6] = mu; sh[1][threadIdx.x >> 6] = mi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < UPD_WAVES; k++) { mu = max(mu, sh[0][k]); mi = max(mi, sh[1][k]); }
        if (mu >= 0) atomicMax(&bounds[0], mu);
        if (mi >= 0) atomicMax(&bounds[1], mi);
    }
}

// the live writes behind the survivors, in batch order
__global__ void k_upd_append(int32_t n, const int32_t* __restrict__ user, const int32_t* __restrict__ item, const float* __restrict__ score,
                             const uint32_t* __restrict__ live_at, const uint32_t* __restrict__ live_incl, int64_t first, int32_t* __restrict__ out_user,
                             int32_t* __restrict__ out_item, float* __restrict__ out_score, int32_t* __restrict__ bounds) {
    int32_t mu = -1, mi = -1;
    bool not_half = false;
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x)
        if (live_at[t]) {
            const int64_t at = first + live_incl[t] - 1;
            const int32_t u = user[t], i = item[t];
            const float s = score[t];
            out_user[at] = u;
            out_item[at] = i;
            out_score[at] = s;
            mu = max(mu, u);
            mi = max(mi, i);
            if (s == s && __half2float(__float2half(s)) != s) not_half = true;
        }
    if (not_half) bounds[2] = 1;
    if (mu >= 0) atomicMax(&bounds[0], mu);                      // at most one pair per live write: the batch is small
    if (mi >= 0) atomicMax(&bounds[1], mi);
}

// counters[0..3] = replaced, inserted, deleted, delete_missed over the table's keys
__global__ void k_upd_counters(int32_t m, const uint32_t* __restrict__ tpos, const uint32_t* __restrict__ live_at, const uint32_t* __restrict__ matched,
                               unsigned long long* __restrict__ counters) {
    const int32_t m_up = (m + 63) & ~63;                        // whole waves enter every ballot
    unsigned long long c[4] = {0, 0, 0, 0};
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < m_up; t += gridDim.x * blockDim.x) {
        int kind = -1;
        if (t < m) kind = (live_at[tpos[t]] ? 0 : 2) + (matched[t] ? 0 : 1);
#pragma unroll
        for (int k = 0; k < 4; k++) c[k] += __popcll(__ballot(kind == k));
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 4; k++)
            if (c[k]) atomicAdd(&counters[k], c[k]);
}

}  // namespace

fy_ratings* ratings_apply(Context* ctx, const fy_ratings* R, int64_t n, const int32_t* user, const int32_t* item, const float* score,
                          const uint8_t* remove, int location, fy_ratings_update_stats* stats) {
    if (n > INT32_MAX) FY_FAIL(FY_ERR_UNSUPPORTED, "a batch of %lld writes: at most 2^31 - 1", (long long)n);
    const int64_t nnz = R->nnz;
    fy_ratings_update_stats st{};
    st.n_writes = n;
    std::unique_ptr<fy_ratings> out(new fy_ratings);
    out->ctx = ctx;

    if (n == 0) {   // a copy
        out->nnz = nnz;
        out->user.alloc(ctx, (size_t)nnz);
        out->item.alloc(ctx, (size_t)nnz);
        out->score.alloc(ctx, (size_t)nnz);
        d2d(ctx, out->user.get(), R->user.get(), (size_t)nnz);
        d2d(ctx, out->item.get(), R->item.get(), (size_t)nnz);
        d2d(ctx, out->score.get(), R->score.get(), (size_t)nnz);
        out->max_user = R->max_user;
        out->max_item = R->max_item;
        out->scores_fp16_exact = R->scores_fp16_exact;
        sync(ctx);
        st.nnz_out = nnz;
        if (stats) *stats = st;
        return out.release();
    }

    hipStream_t sm = ctx->stream;
    const int32_t nb = (int32_t)n;
    // ---- the batch in HBM
    DevBuf<int32_t> up_user, up_item;
    DevBuf<float> up_score;
    DevBuf<uint8_t> up_remove;
    SyncOnUnwind drain(sm);             // the caller's arrays are the sources of the queued uploads
    if (location == FY_HOST) {
        up_user.alloc(ctx, (size_t)n);
        up_item.alloc(ctx, (size_t)n);
        up_score.alloc(ctx, (size_t)n);
        h2d(ctx, up_user.get(), user, (size_t)n);
        h2d(ctx, up_item.get(), item, (size_t)n);
        h2d(ctx, up_score.get(), score, (size_t)n);
        user = up_user.get(); item = up_item.get(); score = up_score.get();
        if (remove) {
            up_remove.alloc(ctx, (size_t)n);
            h2d(ctx, up_remove.get(), remove, (size_t)n);
            remove = up_remove.get();
        }
    }
    // ---- table of distinct keys (last write each), user bitmap, live flags by batch position
    DevBuf<uint64_t> keys(ctx, (size_t)n), skeys(ctx, (size_t)n), tkeys(ctx, (size_t)n);
    DevBuf<uint32_t> pos(ctx, (size_t)n), spos(ctx, (size_t)n), tpos(ctx, (size_t)n), is_last(ctx, (size_t)n), run_incl(ctx, (size_t)n),
        live_at(ctx, (size_t)n), live_incl(ctx, (size_t)n), bitmap(ctx, UPD_BITMAP_WORDS);
    bitmap.zero();
    k_upd_pack<<<small_grid(n), 256, 0, sm>>>(nb, user, item, keys.get(), pos.get(), bitmap.get());
    FY_KERNEL_CHECK();
    sort_pairs_u64_u32(ctx, keys.get(), skeys.get(), pos.get(), spos.get(), (size_t)n);      // stable: a run keeps the batch order
    k_upd_runs<<<small_grid(n), 256, 0, sm>>>(nb, skeys.get(), spos.get(), remove, is_last.get(), live_at.get());
    FY_KERNEL_CHECK();
    inclusive_scan_u32(ctx, is_last.get(), run_incl.get(), (size_t)n);
    inclusive_scan_u32(ctx, live_at.get(), live_incl.get(), (size_t)n);
    k_upd_table<<<small_grid(n), 256, 0, sm>>>(nb, skeys.get(), spos.get(), is_last.get(), run_incl.get(), tkeys.get(), tpos.get());
    FY_KERNEL_CHECK();
    uint32_t h_m = 0, h_live = 0;
    d2h(ctx, &h_m, run_incl.get() + (n - 1), 1);
    d2h(ctx, &h_live, live_incl.get() + (n - 1), 1);
    sync(ctx);
    const int32_t m = (int32_t)h_m;
    const int64_t n_live = h_live;
    st.n_superseded = n - m;

    // ---- the source: count, scan over the waves, write
    DevBuf<uint32_t> matched(ctx, (size_t)m);
    matched.zero();
    DevBuf<int32_t> bounds(ctx, 3);
    FY_HIP(hipMemsetAsync(bounds.get(), 0xFF, 2 * sizeof(int32_t), sm));   // -1
    FY_HIP(hipMemsetAsync(bounds.get() + 2, 0, sizeof(int32_t), sm));
    UpdSource S{};
    int grid = 0;
    size_t lds = 0;
    int64_t n_waves = 0, kept = 0;
    DevBuf<int64_t> wave_count, wave_incl;
    if (nnz) {
        grid = (int)std::max<int64_t>(1, std::min<int64_t>(2 * (int64_t)ctx->num_cus, ceil_div(nnz, (int64_t)UPD_WAVES * UPD_TILE)));
        n_waves = (int64_t)grid * UPD_WAVES;
        S.nnz = nnz;
        S.per = round_up(ceil_div(nnz, n_waves), UPD_TILE);
        S.user = R->user.get(); S.item = R->item.get(); S.score = R->score.get();
        S.bitmap = bitmap.get();
        S.tkeys = tkeys.get();
        S.m = m;
        S.lds_keys = m <= std::min(ctx->tune.upd_lds_keys, UPD_LDS_KEYS_MAX) ? m : 0;
        lds = (size_t)S.lds_keys * sizeof(uint64_t) + UPD_BITMAP_WORDS * sizeof(uint32_t);
        FY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_upd_source<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(UPD_LDS_KEYS_MAX * sizeof(uint64_t) + UPD_BITMAP_WORDS * sizeof(uint32_t))));
        FY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_upd_source<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(UPD_LDS_KEYS_MAX * sizeof(uint64_t) + UPD_BITMAP_WORDS * sizeof(uint32_t))));
        wave_count.alloc(ctx, (size_t)n_waves);
        wave_incl.alloc(ctx, (size_t)n_waves);
        k_upd_source<false><<<grid, UPD_BLOCK, lds, sm>>>(S, matched.get(), wave_count.get(), nullptr, nullptr, nullptr, nullptr, nullptr);
        FY_KERNEL_CHECK();
        inclusive_scan_i64(ctx, wave_count.get(), wave_incl.get(), (size_t)n_waves);
        d2h(ctx, &kept, wave_incl.get() + (n_waves - 1), 1);
        sync(ctx);
    }
    if (kept < 0 || kept > nnz) FY_FAIL(FY_ERR_HIP, "ratings update: %lld survivors of %lld entries", (long long)kept, (long long)nnz);
    const int64_t nnz_out = kept + n_live;
    out->nnz = nnz_out;
    out->user.alloc(ctx, (size_t)nnz_out);
    out->item.alloc(ctx, (size_t)nnz_out);
    out->score.alloc(ctx, (size_t)nnz_out);
    if (nnz) {
        k_upd_source<true><<<grid, UPD_BLOCK, lds, sm>>>(S, nullptr, nullptr, wave_incl.get(), out->user.get(), out->item.get(), out->score.get(),
                                                         bounds.get());
        FY_KERNEL_CHECK();
    }
    k_upd_append<<<small_grid(n), 256, 0, sm>>>(nb, user, item, score, live_at.get(), live_incl.get(), kept, out->user.get(), out->item.get(),
                                                 out->score.get(), bounds.get());
    FY_KERNEL_CHECK();
    DevBuf<unsigned long long> counters(ctx, 4);
    counters.zero();
    k_upd_counters<<<small_grid(m), 256, 0, sm>>>(m, tpos.get(), live_at.get(), matched.get(), counters.get());
    FY_KERNEL_CHECK();
    unsigned long long h_c[4];
    int32_t h_b[3];
    d2h(ctx, h_c, counters.get(), 4);
    d2h(ctx, h_b, bounds.get(), 3);
    sync(ctx);                          // the caller's arrays (host or device) have been read
    out->max_user = nnz_out ? h_b[0] : -1;
    out->max_item = nnz_out ? h_b[1] : -1;
    out->scores_fp16_exact = nnz_out ? h_b[2] == 0 : false;
    st.n_replaced = (int64_t)h_c[0];
    st.n_inserted = (int64_t)h_c[1];
    st.n_deleted = (int64_t)h_c[2];
    st.n_delete_missed = (int64_t)h_c[3];
    st.n_source_dropped = nnz - kept;
    st.nnz_out = nnz_out;
    if (stats) *stats = st;
    return out.release();
}

}  // namespace fy
