// fy_rm2_request.hip -- RM2 on request (fy_rm2_score_users): the lists of the named users, with the work sized by the request.
//
// DESIGN.md section 2b.  With x_vi = r_vi / s_v and i NOT rated by u,
//     sum_{v != u} c_vi c_vj = (1-l)^2 G[j][i] + q_j b_i + a_i e_uj ,      G = X^T X of the cluster,
// a user u reads only the rows G[j][.] of the items j it rated.  The requested users are grouped by cluster; per cluster (and per
// batch that fits fy_rm2_params::workspace_bytes) J = the union of their rated items, and
//   k_req_slab   forms the |J| x I_c slab of those rows in fp64: row j = sum over the raters v of j (column j of the per-cluster CSC)
//                of x_vj * x_v. scattered along v's CSR row.  A workgroup owns a (row j, column chunk) pair and accumulates in LDS in
//                FIXED POINT (64-bit integer adds: the sums do not depend on the order of the atomics, the slab is bit-reproducible);
//                rows are rounded once, to fp64.  Work: sum_{j in J} sum_{v rates j} n_v products instead of sum_v n_v^2.
//   k_req_score  one workgroup per (requested user, 256 candidate columns): lanes own columns, the loop runs over the user's rated
//                items, reads slab[slot_j][i] coalesced, forms the term and adds its log in fp64; pvpi is added, the user's own
//                items are masked (NaN), the row is cast to float and handed to the top-N kernels of the full job (k_topn_*).
// No fp32 / 24-bit storage, no refinement pass, no branch and bound on this path.  A cluster of which more than
// Tuning::req_full_share of the users is asked for is scored by the full pass (fy::rm2_score) and the unrequested rows are dropped.
#include <algorithm>
#include <cmath>
#include <limits>

#include "fy_rm1.hpp"
#include "fy_rm2_request.hpp"

namespace fy {
namespace {

inline int req_grid(int64_t n, int block = 256, int cap = 256 * 16) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, block), cap));
}

constexpr int SLAB_THREADS = 1024;   // 64 groups of 16 lanes, a group walks one rater's row at a time
constexpr int SLAB_GROUP = 16;
constexpr int SCORE_COLS = 256;      // candidate columns of a scoring workgroup (one per lane)

// p(i|C) of every (cluster, item) in rank order: itemsum / totalSum (k_item_coll + k_pair_p of the full job, fp64)
__global__ void k_req_p(int32_t nP, int32_t nI, const int32_t* __restrict__ rank_pair, const int32_t* __restrict__ pair_di,
                        const double* __restrict__ stats, double* __restrict__ p_rank) {
    const double total = stats[nI] / 100.0;
    for (int32_t pos = blockIdx.x * blockDim.x + threadIdx.x; pos < nP; pos += gridDim.x * blockDim.x)
        p_rank[pos] = stats[pair_di[rank_pair[pos]]] / total;
}

// choff[slot * stride + ch] = first entry of the slot's CSR row with column >= ch * CH (ch = stride - 1: the row's end for every cluster)
__global__ void k_req_chunk_offsets(int32_t nU, int32_t CH, int32_t stride, const int32_t* __restrict__ rowptr,
                                    const int32_t* __restrict__ csr_idx, int32_t* __restrict__ choff) {
    const int64_t total = (int64_t)nU * stride;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t s = (int32_t)(t / stride), ch = (int32_t)(t % stride);
        const int32_t a = rowptr[s], b = rowptr[s + 1];
        int32_t lo = a, hi = b;
        const int64_t key = (int64_t)ch * CH;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if ((int64_t)csr_idx[mid] < key) lo = mid + 1; else hi = mid;
        }
        choff[t] = ch == stride - 1 ? b : lo;
    }
}

// Workgroup = (row j of the slab, column chunk).  The accumulators hold round(x_vj x_vi 2^k) with k per row from b_j = sum_v x_vj, an
// upper bound of every entry of the row (x_vi <= 1): b_j 2^k < 2^62, so no sum overflows and a contribution resolves 2^-61 of b_j.
__global__ __launch_bounds__(SLAB_THREADS) void k_req_slab(SlabArgs A) {
    extern __shared__ unsigned long long req_acc[];
    const int32_t row = (int32_t)(blockIdx.x / (unsigned)A.nch), ch = (int32_t)(blockIdx.x % (unsigned)A.nch);
    const int32_t c0 = ch * A.CH, c1 = min(A.Ic, c0 + A.CH), w = c1 - c0;
    for (int32_t t = threadIdx.x; t < w; t += SLAB_THREADS) req_acc[t] = 0ull;
    __syncthreads();
    const int32_t pos = A.pbase + A.J[row];
    const int32_t pr = A.rank_pair[pos];
    const int32_t q0 = A.pair_start[pr], q1 = A.pair_start[pr + 1];
    // (general smoothing: G[j][i] = sum_v (r'_vj / d_v^2) r'_vi <= (sum_v r'_vj / d_v^2) * (largest r' of the cluster))
    int ex = ilogb(A.fx_rank ? (double)A.fx_rank[3 * (int64_t)pos] * A.rmax : A.b_rank[pos]);
    ex = max(-900, min(ex, 60));
    const double scale = ldexp(1.0, 61 - ex), unscale = ldexp(1.0, ex - 61);
    const int g = threadIdx.x / SLAB_GROUP, gl = threadIdx.x % SLAB_GROUP;
    for (int32_t q = q0 + g; q < q1; q += SLAB_THREADS / SLAB_GROUP) {
        const int32_t v = A.csc_slot[q];
        const double inv = 1.0 / A.usum_slot[v];
        const double wgt = (double)A.csc_r[q] * inv * inv * scale;        // r_vj / s_v^2 (scaled), so wgt * r_vi = x_vj x_vi
        const int32_t f0 = A.choff[(int64_t)v * A.stride + ch], f1 = A.choff[(int64_t)v * A.stride + ch + 1];
        for (int32_t f = f0 + gl; f < f1; f += SLAB_GROUP) {
            const int32_t i = A.csr_idx[f] - c0;
            if (i >= 0 && i < w) atomicAdd(&req_acc[i], (unsigned long long)__double2ull_rn(wgt * (double)A.csr_r[f]));
        }
    }
    __syncthreads();
    double* __restrict__ out = A.slab + (int64_t)row * A.ld + c0;
    for (int32_t t = threadIdx.x; t < w; t += SLAB_THREADS) out[t] = (double)req_acc[t] * unscale;
}

struct ScoreReqArgs {
    const int32_t* __restrict__ user_slot;  // [nb] slots of the batch's users
    const int32_t* __restrict__ slotmap;    // [Ic] item index -> slab row (-1: not in the slab)
    const double* __restrict__ slab;
    int64_t ld;
    int32_t Ic, n_chunks;
    const int32_t* __restrict__ rowptr;
    const int32_t* __restrict__ csr_idx;
    const float* __restrict__ csr_r;
    const double* __restrict__ usum_slot;
    const double* __restrict__ p_rank;      // (+ pbase)
    const double* __restrict__ b_rank;      // (+ pbase)
    double lambda, ln_items, ln_users, users_minus_1;
    float* __restrict__ S;
    int64_t ldS;
    int32_t general, cluster;               // general smoothing: b_rank is b~, csr_r r', usum_slot d_v
    SmoothArgs G;
};

__global__ __launch_bounds__(SCORE_COLS) void k_req_score(ScoreReqArgs A) {
    __shared__ double sh_e[SCORE_COLS], sh_q[SCORE_COLS];
    __shared__ int32_t sh_row[SCORE_COLS], sh_j[SCORE_COLS];
    const int32_t u = (int32_t)(blockIdx.x / (unsigned)A.n_chunks), ch = (int32_t)(blockIdx.x % (unsigned)A.n_chunks);
    const int32_t i = ch * SCORE_COLS + (int32_t)threadIdx.x;
    const int32_t slot = A.user_slot[u];
    const int32_t f0 = A.rowptr[slot], f1 = A.rowptr[slot + 1];
    const double s = A.usum_slot[slot];
    const bool live = i < A.Ic;
    double a_i = live ? A.lambda * A.p_rank[i] : 0.0;
    const double b_i = live ? A.b_rank[i] : 0.0;
    double w2 = (1.0 - A.lambda) * (1.0 - A.lambda), w1 = A.lambda * (1.0 - A.lambda);
    if (A.general) { a_i = live ? A.p_rank[i] : 0.0; w2 = 1.0; w1 = 1.0; }      // term = G + p_j b~_i + p_i e~_uj
    double acc = 0.0;
    bool rated = false;
    for (int32_t base = f0; base < f1; base += SCORE_COLS) {       // (block-uniform)
        const int32_t f = base + (int32_t)threadIdx.x;
        if (f < f1) {
            const int32_t j = A.csr_idx[f];
            const double x = (double)A.csr_r[f] / s;
            const double p = A.p_rank[j];
            double e = fy_req_e(A.lambda, A.b_rank[j], x, A.users_minus_1, p);      // = sum_{v != u} c_vj
            if (A.general)
                e = fy_e_general(A.b_rank[j], p, (double)A.csr_r[f], s, (double)A.G.deg_slot[slot], A.G.beta_slot[slot], A.G.s2_cluster[A.cluster],
                                 A.G.bt_scale, A.G.bt_by_n);
            sh_e[threadIdx.x] = e;
            sh_q[threadIdx.x] = w1 * p;
            sh_j[threadIdx.x] = j;
            sh_row[threadIdx.x] = A.slotmap[j];
        }
        __syncthreads();
        const int32_t m = min(SCORE_COLS, f1 - base);
        if (live)
            for (int32_t k = 0; k < m; k++) {
                rated |= sh_j[k] == i;
                const int32_t r = sh_row[k];
                const double g = r >= 0 ? A.slab[(int64_t)r * A.ld + i] : __longlong_as_double(0x7FF8000000000000ll);
                acc += fy_req_log_term(w2, g, sh_q[k], b_i, a_i, sh_e[k]);
            }
        __syncthreads();
    }
    const double n = (double)(f1 - f0);
    A.S[(int64_t)u * A.ldS + i] = live && !rated ? fy_req_row_value(acc, n, A.ln_items, A.ln_users) : __uint_as_float(0x7FC00000u);
}

// rows of the full job's result -> the request's result (one wave per user)
__global__ void k_req_copy_rows(int32_t n, const int32_t* __restrict__ desc /* 3 per user: src, dst, count */,
                                const int32_t* __restrict__ s0, const int32_t* __restrict__ s1, const float* __restrict__ s2, const int32_t* __restrict__ s3,
                                int32_t* __restrict__ d0, int32_t* __restrict__ d1, float* __restrict__ d2, int32_t* __restrict__ d3) {
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int32_t u = blockIdx.x * wpb + (threadIdx.x >> 6); u < n; u += gridDim.x * wpb) {
        const int32_t src = desc[3 * u], dst = desc[3 * u + 1], cnt = desc[3 * u + 2];
        for (int32_t k = lane; k < cnt; k += 64) {
            d0[dst + k] = s0[src + k];
            d1[dst + k] = s1[src + k];
            d2[dst + k] = s2[src + k];
            d3[dst + k] = s3[src + k];
        }
    }
}

}  // namespace

RequestState& rm2_request_state(const RequestView& V) {
    Context* ctx = V.ctx;
    const Prepared& P = *V.P;
    const int32_t CH = ctx->tune.req_chunk;
    auto* S = static_cast<RequestState*>(V.state->get());
    if (S && S->CH == CH) return *S;
    sync(ctx);      // (a state of another chunk width may still be read by a queued kernel)
    V.state->reset();
    std::shared_ptr<RequestState> fresh(new RequestState);
    fresh->CH = CH;
    int64_t max_Ic = 0;
    for (int c = 0; c < P.K; c++) max_Ic = std::max<int64_t>(max_Ic, P.pcstart[c + 1] - P.pcstart[c]);
    fresh->stride = (int32_t)ceil_div(std::max<int64_t>(max_Ic, 1), CH) + 1;
    fresh->uid.resize((size_t)P.nU);
    fresh->du2slot.resize((size_t)P.nU);
    fresh->rowptr.resize((size_t)P.nU + 1);
    fresh->csr_idx.resize((size_t)P.nnz);
    fresh->walk.resize((size_t)P.nP);
    d2h(ctx, fresh->uid.data(), P.uid.get(), (size_t)P.nU);
    d2h(ctx, fresh->du2slot.data(), P.du2slot.get(), (size_t)P.nU);
    d2h(ctx, fresh->rowptr.data(), P.rowptr.get(), (size_t)P.nU + 1);
    d2h(ctx, fresh->csr_idx.data(), P.csr_idx.get(), (size_t)P.nnz);
    d2h(ctx, fresh->walk.data(), V.walk_rank, (size_t)P.nP);
    fresh->choff.alloc(ctx, (size_t)P.nU * (size_t)fresh->stride);
    k_req_chunk_offsets<<<req_grid((int64_t)P.nU * fresh->stride), 256, 0, ctx->stream>>>(P.nU, CH, fresh->stride, P.rowptr.get(), P.csr_idx.get(),
                                                                                          fresh->choff.get());
    FY_KERNEL_CHECK();
    sync(ctx);
    *V.state = fresh;
    return *fresh;
}

void rm2_request_p(const RequestView& V, double* p_rank) {
    const Prepared& P = *V.P;
    k_req_p<<<req_grid(P.nP), 256, 0, V.ctx->stream>>>(P.nP, P.nI, P.rank_pair.get(), P.pair_di.get(), V.stats, p_rank);
    FY_KERNEL_CHECK();
}

void rm2_launch_req_slab(hipStream_t st, const SlabArgs& SA, const char* who) {
    if ((int64_t)SA.nJ * SA.nch > 0x7FFFFFFFll) FY_FAIL(FY_ERR_UNSUPPORTED, "%s: %d slab rows x %d chunks exceed the launch grid", who, SA.nJ, SA.nch);
    FY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_req_slab), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    k_req_slab<<<(unsigned)((int64_t)SA.nJ * SA.nch), SLAB_THREADS, (size_t)SA.CH * sizeof(unsigned long long), st>>>(SA);
    FY_KERNEL_CHECK();
}

namespace {

struct ReqUser {
    int32_t slot, du, cluster, n_out, out_off;
};

}  // namespace

fy_result* rm2_score_users(fy_rm2_job* J, const fy_rm2_request* rq) {
    RequestView V;
    rm2_request_view(J, V);
    if (V.prm.flags & FY_RM2_ESTIMATOR_RM1) return rm1_score_users(V, rq);      // one fp64 pass of its own (fy_rm1.hip)
    Context* ctx = V.ctx;
    const Prepared& P = *V.P;
    const fy_rm2_params& prm = V.prm;
    hipStream_t st = ctx->stream;
    std::unique_ptr<fy_result> R(new fy_result);
    R->ctx = ctx;
    R->kind = 0;
    R->has_request_stats = true;
    R->rq.users_asked = rq->n_users;
    R->st.nnz = P.nnz;
    R->st.n_users = P.nU;
    R->st.n_items = P.nI;
    R->d_user_id.alloc(ctx, 0);
    R->d_item_id.alloc(ctx, 0);
    if (P.nnz == 0 || rq->n_users == 0) return R.release();

    // host buffers of queued uploads live to the end of the call; a failure drains the stream before they go
    std::vector<std::vector<int32_t>> uploads;
    std::unique_ptr<fy_result> full;      // the full job's result, when a cluster takes the full pass
    SyncOnUnwind drain(st);
    EventTimer t_total(ctx), t_tables(ctx), t_cooc(ctx), t_score(ctx), t_topn(ctx);
    const size_t sp_total = t_total.begin();
    const size_t sp_tables = t_tables.begin();
    RequestState& S = rm2_request_state(V);
    DevBuf<double> p_rank(ctx, (size_t)P.nP);
    rm2_request_p(V, p_rank.get());

    // ---- the request: known users of this rank's share, once each, in the order of the unrestricted job (slot order)
    std::vector<std::pair<int32_t, int32_t>> known;      // (slot, dense user index)
    known.reserve((size_t)rq->n_users);
    for (int64_t t = 0; t < rq->n_users; t++) {
        const int32_t raw = rq->users[t];
        if (raw < 0) continue;
        auto it = std::lower_bound(S.uid.begin(), S.uid.end(), raw);
        if (it == S.uid.end() || *it != raw) continue;
        const int32_t du = (int32_t)(it - S.uid.begin()), slot = S.du2slot[(size_t)du];
        if (slot >= V.slot_lo && slot < V.slot_hi) known.emplace_back(slot, du);
    }
    std::sort(known.begin(), known.end());
    known.erase(std::unique(known.begin(), known.end()), known.end());
    R->rq.users_known = (int64_t)known.size();

    // ---- per user: does it get a list, how long (k_user_meta of the full job)
    const int32_t N = prm.number_of_recommendations;
    std::vector<ReqUser> users;
    users.reserve(known.size());
    std::vector<char> touched((size_t)P.K, 0);
    int64_t n_recs = 0, log_terms = 0, max_Ic = 0;
    {
        int c = 0;
        for (size_t k = 0; k < known.size(); k++) {
            const int32_t slot = known[k].first, du = known[k].second;
            while (slot >= P.ucstart[c + 1]) c++;
            touched[(size_t)c] = 1;
            const int32_t Ic = P.pcstart[c + 1] - P.pcstart[c];
            const int32_t n = S.rowptr[(size_t)slot + 1] - S.rowptr[(size_t)slot];
            const int32_t unrated = Ic - n;
            if (unrated <= 0 || S.uid[(size_t)du] < prm.filter_users) continue;      // AbstractRM2Reducer.java:210-213, 221-223
            const int32_t keep = std::max(0, std::min(N, unrated));
            if (n_recs + keep > (int64_t)std::numeric_limits<int32_t>::max()) FY_FAIL(FY_ERR_UNSUPPORTED, "the request's result exceeds 2^31 rows");
            users.push_back(ReqUser{slot, du, c, keep, (int32_t)n_recs});
            n_recs += keep;
            log_terms += (int64_t)n * unrated;
            max_Ic = std::max<int64_t>(max_Ic, Ic);
        }
    }
    for (int c = 0; c < P.K; c++) R->rq.clusters_touched += touched[(size_t)c];
    if (std::min<int64_t>(N, max_Ic) > TOPN_LIST_MAX)
        FY_FAIL(FY_ERR_UNSUPPORTED, "min(numberOfRecommendations, items per cluster) = %d exceeds the top-N kernel limit %d", (int)std::min<int64_t>(N, max_Ic), TOPN_LIST_MAX);
    R->n = n_recs;
    R->st.recs = n_recs;
    R->st.users_scored = (int64_t)users.size();
    R->st.log_terms = log_terms;
    R->d_key0.alloc(ctx, (size_t)n_recs);
    R->d_key1.alloc(ctx, (size_t)n_recs);
    R->d_value.alloc(ctx, (size_t)n_recs);
    R->d_aux.alloc(ctx, (size_t)n_recs);
    const size_t nus = users.size();
    DevBuf<int32_t> d_meta(ctx, 4 * nus + 4);      // [slot][du][n_out][out_off] of the scored users, request order
    if (nus) {
        uploads.emplace_back(4 * nus);
        std::vector<int32_t>& h = uploads.back();
        for (size_t k = 0; k < nus; k++) {
            h[k] = users[k].slot; h[nus + k] = users[k].du; h[2 * nus + k] = users[k].n_out; h[3 * nus + k] = users[k].out_off;
        }
        h2d(ctx, d_meta.get(), h.data(), 4 * nus);
    }
    const int32_t *d_slot = d_meta.get(), *d_du = d_meta.get() + nus, *d_nout = d_meta.get() + 2 * nus, *d_off = d_meta.get() + 3 * nus;
    t_tables.end(sp_tables);

    const int64_t ws = prm.workspace_bytes > 0 ? prm.workspace_bytes : ctx->tune.workspace_default;
    const double share = ctx->tune.req_full_share;
    const double lambda = prm.lambda;
    std::vector<int32_t> full_users;       // positions in `users` of the users of full-pass clusters
    std::vector<int32_t> stamp;            // item index -> slab row of the batch being planned (-1: none)
    DevBuf<int32_t> overflow, any_overflow(ctx, 1);

    for (size_t k0 = 0; k0 < nus;) {
        const int c = users[k0].cluster;
        size_t k1 = k0;
        while (k1 < nus && users[k1].cluster == c) k1++;
        const int32_t Uc = P.csize[(size_t)c], Ic = P.pcstart[c + 1] - P.pcstart[c], pbase = P.pcstart[c];
        if ((double)(k1 - k0) > share * (double)Uc) {      // a large share of the cluster: the full pass, unrequested rows dropped
            for (size_t k = k0; k < k1; k++) full_users.push_back((int32_t)k);
            R->rq.full_pass_clusters++;
            k0 = k1;
            continue;
        }
        const int64_t ld = round_up(Ic, 32), ldS = round_up(Ic, SCORE_COLS);
        const int32_t CH = (int32_t)std::min<int64_t>(S.CH, round_up(Ic, 64)), nch = (int32_t)ceil_div(Ic, CH);
        const int64_t max_rows = ws / (ld * 8);
        // ---- batches of users whose union J fits the slab
        for (size_t b0 = k0; b0 < k1;) {
            stamp.assign((size_t)Ic, -1);
            std::vector<int32_t> rows;
            size_t b1 = b0;
            for (; b1 < k1; b1++) {
                const int32_t slot = users[b1].slot;
                const int32_t f0 = S.rowptr[(size_t)slot], f1 = S.rowptr[(size_t)slot + 1];
                int64_t fresh_rows = 0;
                for (int32_t f = f0; f < f1; f++) fresh_rows += stamp[(size_t)S.csr_idx[(size_t)f]] < 0;
                if ((int64_t)rows.size() + fresh_rows > max_rows) {
                    if (b1 == b0)
                        FY_FAIL(FY_ERR_OUT_OF_MEMORY, "fy_rm2_score_users: the %lld matrix rows of user %d alone (%lld bytes) exceed workspace_bytes = %lld",
                                (long long)fresh_rows, S.uid[(size_t)users[b1].du], (long long)(fresh_rows * ld * 8), (long long)ws);
                    break;
                }
                for (int32_t f = f0; f < f1; f++) {
                    const int32_t j = S.csr_idx[(size_t)f];
                    if (stamp[(size_t)j] < 0) { stamp[(size_t)j] = (int32_t)rows.size(); rows.push_back(j); }
                }
            }
            const int32_t nJ = (int32_t)rows.size(), nb_all = (int32_t)(b1 - b0);
            R->rq.batches++;
            R->rq.slab_rows += nJ;
            R->rq.slab_bytes_peak = std::max<int64_t>(R->rq.slab_bytes_peak, (int64_t)nJ * ld * 8);
            for (int32_t j : rows) R->rq.slab_pair_contribs += S.walk[(size_t)pbase + (size_t)j];
            R->st.cooc_matrix_bytes += (int64_t)nJ * Ic * 8;
            // one upload: [rows of the slab][item -> slab row]
            uploads.emplace_back();
            std::vector<int32_t>& h = uploads.back();
            h.reserve((size_t)nJ + (size_t)Ic);
            h.insert(h.end(), rows.begin(), rows.end());
            h.insert(h.end(), stamp.begin(), stamp.end());
            DevBuf<int32_t> d_plan(ctx, h.size());
            h2d(ctx, d_plan.get(), h.data(), h.size());
            DevBuf<double> slab(ctx, (size_t)nJ * (size_t)ld);
            const size_t sp_c = t_cooc.begin();
            SlabArgs SA{d_plan.get(), nJ, Ic, CH, nch, pbase, S.stride, ld, P.rank_pair.get(), P.pair_start.get(), P.csc_slot.get(), P.csc_r.get(),
                        S.choff.get(), P.csr_idx.get(), P.csr_r.get(), V.usum_slot, V.b_rank, slab.get(),
                        V.general ? V.fx_rank : nullptr, V.general ? (double)V.fx_bounds[3 * (size_t)c + 2] : 0.0};
            rm2_launch_req_slab(st, SA, "fy_rm2_score_users");
            t_cooc.end(sp_c);
            R->st.cooc_launches++;
            // ---- scoring + top-N in groups of users whose float rows fit 256 MB
            const int32_t G = (int32_t)std::max<int64_t>(1, std::min<int64_t>(nb_all, ((int64_t)256 << 20) / (ldS * 4)));
            DevBuf<float> Srows(ctx, (size_t)G * (size_t)ldS);
            if (overflow.size() < (size_t)G) overflow.alloc(ctx, (size_t)G);
            const int32_t n_chunks = (int32_t)(ldS / SCORE_COLS);
            for (int32_t g0 = 0; g0 < nb_all; g0 += G) {
                const int32_t nb = std::min(G, nb_all - g0);
                const size_t first = b0 + (size_t)g0;
                const size_t sp_s = t_score.begin();
                ScoreReqArgs A{d_slot + first, d_plan.get() + nJ, slab.get(), ld, Ic, n_chunks, P.rowptr.get(), P.csr_idx.get(), P.csr_r.get(), V.usum_slot,
                               p_rank.get() + pbase, V.b_rank + pbase, lambda, std::log((double)prm.number_of_items), std::log((double)Uc),
                               (double)(Uc - 1), Srows.get(), ldS, V.general ? 1 : 0, c, V.G};
                k_req_score<<<(unsigned)((int64_t)nb * n_chunks), SCORE_COLS, 0, st>>>(A);
                FY_KERNEL_CHECK();
                t_score.end(sp_s);
                R->st.score_launches++;
                const size_t sp_t = t_topn.begin();
                launch_topn_rows(ctx, st, Srows.get(), ldS, Ic, nb, d_nout + first, d_off + first, P.rank_item_raw.get() + pbase, d_du, P.uid.get(),
                                 (int32_t)first, c, R->d_key0.get(), R->d_key1.get(), R->d_value.get(), R->d_aux.get(), overflow.get(),
                                 any_overflow.get(), N);
                t_topn.end(sp_t);
            }
            b0 = b1;
        }
        k0 = k1;
    }

    // ---- clusters that take the full pass: the full job once, then the requested users' rows
    if (!full_users.empty()) {
        full.reset(rm2_score(J));
        // a user's first row in the full result, by its user column (rows are grouped by user)
        const int64_t fn = full->n;
        std::vector<int32_t> fu((size_t)fn);
        d2h(ctx, fu.data(), full->d_key0.get(), (size_t)fn);
        sync(ctx);
        std::vector<std::pair<int32_t, int32_t>> first_row;      // (raw user id, first row)
        for (int64_t r = 0; r < fn; r++)
            if (r == 0 || fu[(size_t)r] != fu[(size_t)r - 1]) first_row.emplace_back(fu[(size_t)r], (int32_t)r);
        std::sort(first_row.begin(), first_row.end());
        uploads.emplace_back(3 * full_users.size());
        std::vector<int32_t>& desc = uploads.back();
        for (size_t q = 0; q < full_users.size(); q++) {
            const ReqUser& u = users[(size_t)full_users[q]];
            const int32_t raw = S.uid[(size_t)u.du];
            auto it = std::lower_bound(first_row.begin(), first_row.end(), std::make_pair(raw, (int32_t)0));
            if (u.n_out > 0 && (it == first_row.end() || it->first != raw)) FY_FAIL(FY_ERR_STATE, "internal: user %d has no rows in the full pass", raw);
            desc[3 * q] = u.n_out > 0 ? it->second : 0; desc[3 * q + 1] = u.out_off; desc[3 * q + 2] = u.n_out;
        }
        DevBuf<int32_t> d_desc(ctx, desc.size());
        h2d(ctx, d_desc.get(), desc.data(), desc.size());
        const size_t sp_t = t_topn.begin();
        k_req_copy_rows<<<req_grid((int64_t)full_users.size() * 64, 256), 256, 0, st>>>((int32_t)full_users.size(), d_desc.get(), full->d_key0.get(), full->d_key1.get(),
                                                                                   full->d_value.get(), full->d_aux.get(), R->d_key0.get(), R->d_key1.get(),
                                                                                   R->d_value.get(), R->d_aux.get());
        FY_KERNEL_CHECK();
        t_topn.end(sp_t);
        sync(ctx);      // (d_desc and the full result are released below)
    }
    t_total.end(sp_total);
    sync(ctx);
    full.reset();
    R->st.pair_contribs = R->rq.slab_pair_contribs;
    R->st.ms_tables = t_tables.total_ms();
    R->st.ms_cooc = t_cooc.total_ms();
    R->st.ms_score = t_score.total_ms();
    R->st.ms_topn = t_topn.total_ms();
    R->st.ms_total = t_total.total_ms();
    return R.release();
}

}  // namespace fy
