// fy_itemsim_request.hip -- item similarity on request (fy_itemsim_rows): the rows of the named items of a prepared job, with the
// work sized by the request.
//
// DESIGN.md section 2c.  Row j of the similarity matrix needs d_ji = sum_v w_vj w_vi over the raters v of j only: column j of the
// CSC names them, and each rater's CSR row is scattered into the row's accumulators -- the walk of k_req_slab (fy_rm2_request.hip).
//   k_isim_req_rows  workgroup = (requested row j, column chunk).  LDS: CH 64-bit FIXED-POINT accumulators (integer adds: the sums
//                    do not depend on the order of the atomics, requests are bit-reproducible) + the candidate buffer.  Groups of
//                    16 lanes take one rater at a time; the slice of the rater's row inside the chunk comes from the offsets kept
//                    at prepare.  Then the accumulators are read back as fp64 and streamed through the running top-K of the full
//                    build (isim_candidate, isim_append, isim_cut, isim_finish_list: fy_itemsim_kernels.hpp), 1024 columns a step;
//                    the chunk's K best are left as composites with the ordered key.
//   k_isim_merge     (the full build's) folds a row's chunks; k_isim_compact (shared too) writes the result in popularity order.
// Which instantiation a measure takes -- its weight, its finish -- comes from fy_itemsim_plan.hpp (isim_measure, isim_dispatch).
// Nothing here launches or loops over the ratings or over all users: ids are mapped by a binary search per requested id in the
// job's sorted raw ids (host), marking / deduplication / ordering sort the <= n row indices.
#include <algorithm>
#include <cmath>
#include <limits>

#include "fy_itemsim_kernels.hpp"
#include "fy_itemsim_request.hpp"

namespace fy {
namespace {

constexpr int ROWS_THREADS = 1024;   // 64 groups of 16 lanes, a group walks one rater's row at a time
constexpr int ROWS_GROUP = 16;

struct ReqRowsArgs {
    const int32_t* __restrict__ rows;       // [n] popularity ranks of the batch's rows, ascending
    int32_t Ic, CH, nch;
    const int32_t* __restrict__ rank_pair;
    const int32_t* __restrict__ pair_start;
    const int32_t* __restrict__ csc_slot;
    const float* __restrict__ csc_r;
    const int32_t* __restrict__ choff;      // [nU * (nch + 1)]
    const int32_t* __restrict__ csr_idx;
    const float* __restrict__ csr_r;
    const double* __restrict__ csr_w;       // Pearson: centred, normalised preference per CSR entry
    const double* __restrict__ centre;      // Pearson, pair order
    const double* __restrict__ cnorm;
    const double* __restrict__ bound;       // rank order
};

// The accumulators hold round(w_vj w_vi 2^k), k per row from bound[j] >= |d_ji| for every i: bound 2^k < 2^62, so no sum leaves the
// signed 64-bit range, and negative contributions (preferences <= 0, Pearson's centred weights) add modulo 2^64 and read back
// signed.  Exact whenever every product is a multiple of 2^-k' with k' <= k (half stars: k' = 2; the count measures: 0).
template <int M, int W>
__global__ __launch_bounds__(ROWS_THREADS) void k_isim_req_rows(ReqRowsArgs A, ISimEpilogue E) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long isim_req_lds[];      // [CH accumulators][E.cap candidates]
    unsigned long long* acc = isim_req_lds;
    uint64_t* cand = reinterpret_cast<uint64_t*>(isim_req_lds + A.CH);
    __shared__ uint32_t sh_cnt, sh_tau, sh_aux[2], hist[256];
    const int tid = threadIdx.x;
    const int32_t mine = (int32_t)(blockIdx.x / (unsigned)A.nch), ch = (int32_t)(blockIdx.x % (unsigned)A.nch);
    const int32_t row = A.rows[mine];
    const int32_t c0 = ch * A.CH, ncol = min(A.CH, A.Ic - c0);
    for (int32_t t = tid; t < ncol; t += ROWS_THREADS) acc[t] = 0ull;
    if (tid == 0) { sh_cnt = 0; sh_tau = 0; }
    __syncthreads();
    const int32_t pr = A.rank_pair[row];
    const int32_t q0 = A.pair_start[pr], q1 = A.pair_start[pr + 1];
    int ex = ilogb(A.bound[row]);
    ex = max(-900, min(ex, 60));
    const double scale = ldexp(1.0, 61 - ex), unscale = ldexp(1.0, ex - 61);
    double centre = 0.0, inv_cnorm = 0.0;
    bool walk = true;
    if constexpr (W == ISIM_W_PEARSON) {
        centre = A.centre[pr];
        const double cn = A.cnorm[pr];
        walk = cn != 0.0;                       // a constant item has no row (block-uniform)
        inv_cnorm = walk ? 1.0 / cn : 0.0;
    }
    if (walk) {
        const int g = tid / ROWS_GROUP, gl = tid % ROWS_GROUP;
        const int64_t stride = (int64_t)A.nch + 1;
        for (int32_t q = q0 + g; q < q1; q += ROWS_THREADS / ROWS_GROUP) {
            const int32_t v = A.csc_slot[q];
            double wj = scale;
            if constexpr (W == ISIM_W_RATING) wj = (double)A.csc_r[q] * scale;
            if constexpr (W == ISIM_W_PEARSON) wj = (((double)A.csc_r[q] - centre) * inv_cnorm) * scale;
            const int32_t f0 = A.choff[(int64_t)v * stride + ch], f1 = A.choff[(int64_t)v * stride + ch + 1];
            for (int32_t f = f0 + gl; f < f1; f += ROWS_GROUP) {
                const int32_t i = A.csr_idx[f] - c0;
                double wi = 1.0;
                if constexpr (W == ISIM_W_RATING) wi = (double)A.csr_r[f];
                if constexpr (W == ISIM_W_PEARSON) wi = A.csr_w[f];
                if (i >= 0 && i < ncol) atomicAdd(&acc[i], (unsigned long long)__double2ll_rn(wj * wi));
            }
        }
    }
    __syncthreads();
    // the accumulators as fp64 (bit patterns), in place
    for (int32_t t = tid; t < ncol; t += ROWS_THREADS) acc[t] = (unsigned long long)__double_as_longlong((double)(long long)acc[t] * unscale);
    __syncthreads();
    // The full build's running top-K, one step of ROWS_THREADS columns at a time: a candidate must reach the key sh_tau, the buffer
    // is cut back to the K best (isim_cut raises sh_tau) whenever the next step might not fit.  Exact for any input.
    const double scale_row = isim_row_scale<M>(E, row);
    for (int32_t base = 0; base < ncol; base += ROWS_THREADS) {
        const int32_t t = base + tid;
        bool want = false;
        uint64_t c = 0;
        if (t < ncol) {
            const int32_t col = c0 + t;
            uint32_t key;
            const bool ok = isim_candidate<M>(E, __longlong_as_double((long long)acc[t]), scale_row, row, col, key);
            want = ok && key >= sh_tau;
            if (want) c = isim_composite(key, E.rank_item_raw[col]);
        }
        isim_append<false>(cand, &sh_cnt, 0, want, c);      // (fits: sh_cnt + ROWS_THREADS <= cap before the step)
        __syncthreads();
        const uint32_t have = sh_cnt;
        __syncthreads();      // everybody has read the count before the next step's atomics move it
        if (have + ROWS_THREADS > (uint32_t)E.cap) isim_cut(cand, E.K, E.cap, hist, &sh_cnt, &sh_tau, sh_aux);      // block-uniform
    }
    const int keep = isim_finish_list(cand, E.K, hist, &sh_cnt, &sh_tau, sh_aux);
    const int64_t slot = (int64_t)mine * A.nch + ch;
    if (tid == 0) E.part_cnt[slot] = keep;
    for (int i = tid; i < keep; i += ROWS_THREADS) E.part[slot * E.K + i] = cand[i];
}

using RowsKernel = void (*)(ReqRowsArgs, ISimEpilogue);
// the instantiation of a measure: its finish (the template measure), and its weight -- fixed by a finishing measure, one of the three
// where the dot product is the similarity
RowsKernel rows_kernel(int similarity) {
    const int weight = isim_measure(similarity).weight;
    return isim_dispatch(similarity, [&](auto M) -> RowsKernel {
        constexpr int m = decltype(M)::value;
        if constexpr (m != FY_SIMILARITY_COSINE) return k_isim_req_rows<m, isim_measure(m).weight>;
        else return weight == ISIM_W_RATING ? k_isim_req_rows<m, ISIM_W_RATING> : weight == ISIM_W_ONE ? k_isim_req_rows<m, ISIM_W_ONE> : k_isim_req_rows<m, ISIM_W_PEARSON>;
    });
}

}  // namespace

// The rows of the similarity matrix with the popularity ranks rows[0 .. n) (device, ascending), in batches: the row kernel, then the
// merge of each row's chunks into cnt[m] / other[m * K ..] / sim[m * K ..] (raw item ids, best first).  Shared by fy_itemsim_rows and
// the item-CF request pass (fy_itemcf_request.hip).  Returns the number of batches (launches of the row kernel).
int64_t itemsim_build_rank_rows(fy_itemsim_job* J, const int32_t* rows, int64_t n, int32_t* cnt, int32_t* other, float* sim,
                                EventTimer& t_cooc, EventTimer& t_topn) {
    Context* ctx = J->ctx;
    const Prepared& P = J->P;
    const fy_itemsim_params& prm = J->prm;
    hipStream_t st = ctx->stream;
    const int32_t K = prm.max_similarities_per_item, Ic = P.nP, nch = J->nch, CH = J->CH;
    // rows per batch: the per-(row, chunk) partial lists fit the workspace default, the grid fits a launch
    const Tuning& tune = ctx->tune;
    int64_t per_batch = std::max<int64_t>(1, tune.workspace_default / ((int64_t)nch * K * 8));
    per_batch = std::min<int64_t>(per_batch, 0x7FFFFFFFll / nch);
    if (tune.isim_req_rows > 0) per_batch = std::min<int64_t>(per_batch, tune.isim_req_rows);
    per_batch = std::min(per_batch, n);
    DevBuf<int32_t> part_cnt(ctx, (size_t)per_batch * nch);
    DevBuf<uint64_t> part(ctx, (size_t)per_batch * nch * K);
    SyncOnUnwind drain(st);      // a failure in the loop drains the stream before the partial lists go
    int64_t batches = 0;

    const IsimMeasure m = isim_measure(prm.similarity);
    const int cap = ISIM_CAP;
    const size_t lds = (size_t)CH * 8 + (size_t)cap * 8;
    const RowsKernel kernel = rows_kernel(prm.similarity);
    FY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int64_t b0 = 0; b0 < n; b0 += per_batch) {
        const int32_t nb = (int32_t)std::min<int64_t>(per_batch, n - b0);
        ReqRowsArgs A{rows + b0, Ic, CH, nch, P.rank_pair.get(), P.pair_start.get(), P.csc_slot.get(), P.csc_r.get(), J->choff.get(),
                      P.csr_idx.get(), P.csr_r.get(), J->csr_w.get(), J->centre.get(), J->cnorm.get(), J->bound.get()};
        ISimEpilogue E{P.rank_item_raw.get(), K, prm.exclude_self, prm.has_threshold, (float)prm.threshold, prm.rank, prm.world, nullptr, nullptr,
                       nullptr, (m.inv_norm || m.weight == ISIM_W_PEARSON) ? J->inv_norm.get() : nullptr, m.finishes ? J->aux.get() : nullptr, (double)P.nU, part_cnt.get(),
                       part.get(), 0, 0, cap};
        const unsigned grid = (unsigned)((int64_t)nb * nch);
        const size_t sp_c = t_cooc.begin();
        kernel<<<grid, ROWS_THREADS, lds, st>>>(A, E);
        FY_KERNEL_CHECK();
        t_cooc.end(sp_c);
        const size_t sp_t = t_topn.begin();
        k_isim_merge<<<std::min(nb, ctx->num_cus * 8), 256, 0, st>>>(nb, nch, K, part_cnt.get(), part.get(), cnt + b0, other + b0 * K, sim + b0 * K);
        FY_KERNEL_CHECK();
        t_topn.end(sp_t);
        batches++;
    }
    return batches;
}

fy_result* itemsim_rows(fy_itemsim_job* J, const fy_itemsim_request* rq) {
    Context* ctx = J->ctx;
    const Prepared& P = J->P;
    const fy_itemsim_params& prm = J->prm;
    hipStream_t st = ctx->stream;
    std::unique_ptr<fy_result> R = isim_empty_result(ctx, P);
    R->has_itemsim_request_stats = true;
    R->irq.items_asked = rq->n_items;
    R->irq.chunks = J->nch;
    if (P.nnz == 0 || rq->n_items == 0) return R.release();

    // ---- the request: known items of this rank's shard, once each, in the order of the full build (popularity rank)
    std::vector<int32_t> rows;
    rows.reserve((size_t)rq->n_items);
    for (int64_t t = 0; t < rq->n_items; t++) {
        const int32_t raw = rq->items[t];
        if (raw < 0) continue;
        auto it = std::lower_bound(J->raw_sorted.begin(), J->raw_sorted.end(), raw);
        if (it == J->raw_sorted.end() || *it != raw) continue;
        const int32_t r = J->rank_of_sorted[(size_t)(it - J->raw_sorted.begin())];
        if (r % prm.world == prm.rank) rows.push_back(r);
    }
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    const int64_t n = (int64_t)rows.size();
    R->irq.items_known = n;
    for (int32_t r : rows) R->irq.pair_contribs += J->walk[(size_t)r];
    R->st.pair_contribs = R->irq.pair_contribs;
    if (n == 0) return R.release();

    const int32_t K = prm.max_similarities_per_item;
    if (n * K > (int64_t)std::numeric_limits<int32_t>::max()) FY_FAIL(FY_ERR_UNSUPPORTED, "the request's result may exceed 2^31 rows");

    EventTimer t_total(ctx), t_cooc(ctx), t_topn(ctx);
    DevBuf<int32_t> d_rows(ctx, (size_t)n), cnt(ctx, (size_t)n + 1), off(ctx, (size_t)n + 1), other(ctx, (size_t)n * K);
    DevBuf<float> sim(ctx, (size_t)n * K);
    std::vector<int32_t> h_cnt((size_t)n);
    // behind the host ends of the queued copies (`rows`, `h_cnt`) AND the scratch buffers: a failure drains the stream before any of
    // them goes (objects die in reverse order of declaration)
    SyncOnUnwind drain(st);
    const size_t sp_total = t_total.begin();
    h2d(ctx, d_rows.get(), rows.data(), (size_t)n);
    cnt.zero();
    R->irq.batches = itemsim_build_rank_rows(J, d_rows.get(), n, cnt.get(), other.get(), sim.get(), t_cooc, t_topn);
    const size_t sp_t = t_topn.begin();
    exclusive_scan_i32(ctx, cnt.get(), off.get(), (size_t)n + 1);
    d2h(ctx, h_cnt.data(), cnt.get(), (size_t)n);
    const int64_t n_out = fetch(ctx, off.get() + n);
    for (int32_t c : h_cnt) R->irq.rows_emitted += c > 0;
    isim_result_rows(R.get(), n_out);
    if (n_out > 0) {
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n * 64, 256), 256 * 16));
        k_isim_compact<<<grid, 256, 0, st>>>((int32_t)n, K, d_rows.get(), 0, 0, cnt.get(), off.get(), other.get(), sim.get(), P.rank_item_raw.get(),
                                             R->d_key0.get(), R->d_key1.get(), R->d_value.get(), R->d_aux.get());
        FY_KERNEL_CHECK();
    }
    t_topn.end(sp_t);
    t_total.end(sp_total);
    sync(ctx);      // the scratch of this call goes back to the allocator
    R->st.recs = n_out;
    R->st.cooc_launches = R->irq.batches;
    R->st.ms_cooc = t_cooc.total_ms();
    R->st.ms_topn = t_topn.total_ms();
    R->st.ms_total = t_total.total_ms();
    return R.release();
}

}  // namespace fy
