// fy_itemcf_estimate.hip -- item-based CF: the estimated preference of named (user, item) pairs on a prepared similarity job
// (fy_itemcf_estimate_prepared / fy_itemcf_estimate_ratings; include/filmyou.h).
//
// estimate(u, i) is the cell (u, i) of the list pass (k_icf_accumulate + k_icf_finalize, fy_itemcf.hip) before the top-N.  The list
// pass pays a dense accumulator row over the catalogue per user; here the work is sized by the pairs asked for.  The opening, the
// steps from the pairs to the TARGETS (the distinct (known user, known item) pairs, a user's adjacent, columns ascending) and the
// closing are fy_itemcf_pairs.hip, shared with the explanations of fy_itemcf_because.hip; this file keeps
//   chunks               a user's targets are cut into chunks of at most CH (FY_ICF_EST_CHUNK)
//   k_icf_estimate       ONE WAVE per (user, chunk).  LDS per wave: the chunk's columns (ascending), fp64 num / den, int cnt, own flag.
//                        The wave walks the user's kept preferences in CSR order; the 64 lanes stride over row j's entries, each lane
//                        binary-searches its entry's column among the chunk's columns and, on a hit, adds to that target's cells
//                        with plain LDS read-modify-writes.  Then icf_estimate_finish and the scatter to every place of the key.
// Why the bits are the list pass's: a cell receives pd * s (rounded product, then rounded sum: the atomicAdd of a product there, the
// explicit __dmul_rn / __dadd_rn here), |s| and 1 once per contributing preference, in the order of the user's preferences.  The
// rows walked per (user, chunk) are the user's kept rows: the work model is fy_itemcf_estimate_stats.row_entries_walked.
#include "fy_itemcf_pairs.hpp"

namespace fy {
namespace {

constexpr int EST_AGG = 10;      // status counts [0 .. 7], users with an OK pair [8], row entries walked [9]

// target m opens a chunk iff its distance from the first target of its user is a multiple of CH
__global__ void k_est_chunk_heads(int32_t nT, const uint64_t* __restrict__ tkey, int32_t CH, uint32_t* __restrict__ chead) {
    for (int32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < nT; m += gridDim.x * blockDim.x) {
        const uint64_t first_key = tkey[m] & 0xFFFFFFFF00000000ull;
        chead[m] = (m - fy_lower_bound(tkey, 0, m, first_key)) % CH == 0;
    }
}
__global__ void k_est_chunks(int32_t nT, const uint32_t* __restrict__ chead, const uint32_t* __restrict__ cincl, int32_t* __restrict__ cstart) {
    for (int32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < nT; m += gridDim.x * blockDim.x) {
        if (chead[m]) cstart[cincl[m] - 1] = m;
        if (m == nT - 1) cstart[cincl[m]] = nT;
    }
}

struct EstArgs : IcfPairArgs {              // (K .. splace: in both kernels' structs, at the offsets the kernels were tuned with)
    int32_t K, boolean_data, n_chunks, ld;  // ld: targets a wave has room for (the chunk size rounded up to even)
    const int32_t* __restrict__ cstart;     // n_chunks + 1
    const uint64_t* __restrict__ tkey;
    const int32_t* __restrict__ tfirst;     // targets + 1
    const uint32_t* __restrict__ splace;    // place in the input of every sorted entry
    float* __restrict__ o_value;
    int32_t* __restrict__ o_aux;
    long long* __restrict__ walked;         // per chunk
    int32_t* __restrict__ chunk_ok;         // per chunk: one of its targets is FY_ESTIMATE_OK
};

// the LDS writes of the wave's lanes so far are visible to every lane's reads behind this point (one wave: its DS operations are
// executed in the order issued; this keeps the compiler from moving them across)
__device__ __forceinline__ void est_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// position of column c among the chunk's ascending columns, -1 when it is none of them
__device__ __forceinline__ int32_t est_find(const int32_t* col, int32_t nt, int32_t c) {
    const int32_t lo = fy_lower_bound(col, 0, nt, c);
    return (lo < nt && col[lo] == c) ? lo : -1;
}

__global__ void __launch_bounds__(256) k_icf_estimate(EstArgs A) {
    extern __shared__ double est_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int32_t c = blockIdx.x * 4 + w;
    if (c >= A.n_chunks) return;                                 // (no workgroup barrier below: the waves are independent)
    // this wave's 28 B per target: num, den (fp64), col, cnt, own (int32)
    double* num = est_lds + (size_t)w * A.ld * 7 / 2;
    double* den = num + A.ld;
    int32_t* col = (int32_t*)(den + A.ld);
    int32_t* cnt = col + A.ld;
    int32_t* own = cnt + A.ld;
    const int32_t m0 = A.cstart[c], nt = A.cstart[c + 1] - m0;
    const int32_t k = (int32_t)(A.tkey[m0] >> 32);
    const int32_t slot = A.list[k];
    const float thr = A.thr[k];
    for (int32_t i = lane; i < nt; i += 64) {
        col[i] = (int32_t)(uint32_t)A.tkey[m0 + i];
        num[i] = 0.0;
        den[i] = 0.0;
        cnt[i] = 0;
        own[i] = 0;
    }
    est_wave_sync();
    long long walked = 0;
    const int32_t f1 = A.rowptr[slot + 1];
    for (int32_t f = A.rowptr[slot]; f < f1; f++) {              // preferences in CSR order; everything but the inner loop is wave-uniform
        const float p = A.csr_r[f];
        if (p < thr) continue;
        const int32_t j = A.csr_idx[f];
        const int32_t n = A.row_cnt[j];
        if (n == 0) continue;                                    // no similarity row: contributes nothing, not even its self entry (k_icf_accumulate)
        walked += n;
        const int32_t t0 = j * A.K;
        const double pd = A.boolean_data ? 1.0 : (double)p;
        // INVARIANT: a row holds a column at most once and the chunk's targets are distinct columns, so within this loop no two lanes
        // touch one cell; between two rows est_wave_sync orders the lanes.  Each cell therefore sees its additions in preference order.
        for (int32_t t = lane; t < n; t += 64) {
            const int32_t i = A.col_other[t0 + t];
            if (i < 0) continue;
            const int32_t h = est_find(col, nt, i);
            if (h < 0) continue;
            const double s = (double)A.sim[t0 + t];
            num[h] = __dadd_rn(num[h], __dmul_rn(pd, s));
            den[h] = __dadd_rn(den[h], fabs(s));
            cnt[h] += 1;
        }
        if (lane == 0) {                                         // the (j, NaN) self entry: the item itself drops out
            const int32_t h = est_find(col, nt, j);
            if (h >= 0) own[h] = 1;
        }
        est_wave_sync();
    }
    // ---- the finish (icf_estimate_finish, fy_itemcf_pairs.hpp) and the row of every asked pair of the target
    bool ok = false;
    for (int32_t i = lane; i < nt; i += 64) {
        float v;
        const int32_t status = icf_estimate_finish(num[i], den[i], cnt[i], own[i] != 0, A.boolean_data, v);
        ok |= status == FY_ESTIMATE_OK;
        for (int32_t q = A.tfirst[m0 + i]; q < A.tfirst[m0 + i + 1]; q++) {
            const uint32_t at = A.splace[q];
            A.o_value[at] = v;
            A.o_aux[at] = status;
        }
    }
    const bool any_ok = __any(ok);
    if (lane == 0) {
        A.walked[c] = walked;
        A.chunk_ok[c] = any_ok;
    }
}

// the walk of all chunks; users with an OK pair: the first chunk of a user (its chunks are adjacent) that holds one
__global__ void k_est_count_chunks(int32_t n_chunks, const int32_t* __restrict__ cstart, const uint64_t* __restrict__ tkey,
                                   const long long* __restrict__ walked, const int32_t* __restrict__ chunk_ok, unsigned long long* __restrict__ agg) {
    unsigned long long users = 0, walk = 0;
    for (int32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += gridDim.x * blockDim.x) {
        walk += (unsigned long long)walked[c];
        if (!chunk_ok[c]) continue;
        const uint64_t user = tkey[cstart[c]] >> 32;
        bool first = true;
        for (int32_t b = c - 1; b >= 0 && first && (tkey[cstart[b]] >> 32) == user; b--) first = !chunk_ok[b];
        users += first;
    }
    for (int o = 32; o > 0; o >>= 1) {
        users += __shfl_down(users, o, 64);
        walk += __shfl_down(walk, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (users) atomicAdd(&agg[8], users);
        if (walk) atomicAdd(&agg[9], walk);
    }
}

}  // namespace

fy_result* itemcf_estimate_prepared(fy_itemsim_job* J, const fy_itemcf_params* prm, int64_t n_all_pairs, const int32_t* users, const int32_t* items,
                                    int location) {
    Context* ctx = J->ctx;
    if (prm->max_prefs_per_user <= 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "maxPrefsPerUser must be > 0");
    int64_t off;
    int32_t n;
    std::unique_ptr<fy_result> Rs = icf_pairs_open(J, prm, n_all_pairs, users, items, location, 4, off, n);
    hipStream_t st = ctx->stream;
    Rs->n = n;
    Rs->has_itemcf_estimate_stats = true;
    fy_itemcf_estimate_stats& es = Rs->est;
    es.pairs_asked = n;
    es.pair_offset = off;
    es.rows_stored = J->store.rows;
    Rs->d_key0.alloc(ctx, (size_t)n);
    Rs->d_key1.alloc(ctx, (size_t)n);
    Rs->d_value.alloc(ctx, (size_t)n);
    Rs->d_aux.alloc(ctx, (size_t)n);
    if (n == 0) return Rs.release();

    IcfrTimers tm(ctx);
    unsigned long long h_agg[EST_AGG] = {};
    SyncOnUnwind drain(st);      // behind the host ends of the queued copies (and the caller's id arrays); the buffers below are released before it drains
    const size_t sp_total = tm.total.begin();
    size_t sp_tab = tm.tables.begin();
    DevBuf<unsigned long long> agg(ctx, EST_AGG);
    agg.zero();
    float* o_value = Rs->d_value.get();
    int32_t* o_aux = Rs->d_aux.get();

    // ---- the front half (fy_itemcf_pairs.hip): known users, their rows in the store, keys, sort, targets
    IcfPairTargets T;
    icf_pair_targets(J, prm->max_prefs_per_user, n, users + off, items + off, location, Rs->d_key0.get(), Rs->d_key1.get(), o_value, o_aux, tm, sp_tab, T, "estimate");
    es.users_known = T.n_known;
    icfr_report(es, T.built, T.n_known > 0);
    const int32_t n_targets = T.n_targets;
    int32_t n_chunks = 0;
    if (n_targets > 0) {
        // ---- chunks
        const int32_t CH = std::max(1, std::min(ctx->tune.icf_est_chunk, ICF_EST_CHUNK_MAX));
        DevBuf<uint32_t> chead(ctx, (size_t)n_targets), cincl(ctx, (size_t)n_targets);
        k_est_chunk_heads<<<grid_for(n_targets), 256, 0, st>>>(n_targets, T.tkey.get(), CH, chead.get());
        FY_KERNEL_CHECK();
        inclusive_scan_u32(ctx, chead.get(), cincl.get(), (size_t)n_targets);
        n_chunks = (int32_t)fetch(ctx, cincl.get() + (n_targets - 1));
        if (n_chunks < 1 || n_chunks > n_targets) FY_FAIL(FY_ERR_HIP, "estimate: %d chunks over %d targets", n_chunks, n_targets);
        DevBuf<int32_t> cstart(ctx, (size_t)n_chunks + 1), chunk_ok(ctx, (size_t)n_chunks);
        DevBuf<long long> walked(ctx, (size_t)n_chunks);
        k_est_chunks<<<grid_for(n_targets), 256, 0, st>>>(n_targets, chead.get(), cincl.get(), cstart.get());
        FY_KERNEL_CHECK();
        tm.tables.end(sp_tab);

        // ---- the estimate kernel: one wave per (user, chunk)
        const size_t sp_score = tm.score.begin();
        EstArgs A{};
        icf_pair_args(A, J, T, prm->boolean_data);
        A.n_chunks = n_chunks; A.ld = (int32_t)round_up(CH, 2); A.cstart = cstart.get();
        A.o_value = o_value; A.o_aux = o_aux; A.walked = walked.get(); A.chunk_ok = chunk_ok.get();
        k_icf_estimate<<<(int)ceil_div((int64_t)n_chunks, (int64_t)4), 256, (size_t)4 * A.ld * 28, st>>>(A);
        FY_KERNEL_CHECK();
        tm.score.end(sp_score);
        k_est_count_chunks<<<grid_for(n_chunks), 256, 0, st>>>(n_chunks, cstart.get(), T.tkey.get(), walked.get(), chunk_ok.get(), agg.get());
        FY_KERNEL_CHECK();
    } else {
        tm.tables.end(sp_tab);
    }
    icf_pairs_close(Rs.get(), n, o_aux, agg, h_agg, es.by_status, T.built, (int64_t)tm.score.count(), tm, sp_total);
    es.targets = n_targets;
    es.chunks = n_chunks;
    es.row_entries_walked = (int64_t)h_agg[9];
    return Rs.release();
}

}  // namespace fy
