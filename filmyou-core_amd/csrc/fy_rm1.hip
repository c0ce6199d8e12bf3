// fy_rm1.hip -- the RM1 estimator (Parapar et al. 2013) on a prepared RM2 job: FY_RM2_ESTIMATOR_RM1, DESIGN.md section 2g.
//
//     score(u, i) = -ln U_c + ln sum_{v in V_c, v != u} c_vi prod_{j in rated(u)} c_vj ,     c_vi = w r'_vi / d_v + beta_v p_i
//
// a log of a sum over neighbours, each weighted by its likelihood of the user's whole profile (e^-1000 and below).  The likelihoods
// are never formed unshifted: with L_uv = sum_j ln c_vj and m_u = max_v L_uv
//     score = -ln U_c + m_u + ln( sum_v exp(L_uv - m_u) c_vi ) .
// Sparse form: e_vj = ln c_vj - ln p_j per kept rating, cnt_uv = |rated(u) & rated(v)|, E_uv = sum of e_vj over the intersection,
// LP_u = sum_{j in rated(u)} ln p_j:
//     L_uv = LP_u + E_uv + (n_u - cnt_uv) ln beta_v                                   (0 * -inf := 0)
//     sum_v w_uv c_vi = p_i sum_v w_uv beta_v + sum_{v rates i} w_uv (w r'_vi / d_v)
// Per touched cluster (once): k_rm1_prep_rows (e, LP, beta, ln beta in CSR order), k_rm1_prep_cols (a_vi = w r'_vi / d_v in CSC order).
// Per batch of users that fits fy_rm2_params::workspace_bytes (weights B x U_c x 8 bytes, scores B x I_c x 4 bytes):
//   k_rm1_loglik   workgroup = (user, chunk of neighbours).  The user's rated set is a bitmask over the cluster's columns in LDS; a wave
//                  takes a neighbour, its lanes stride the neighbour's CSR row, test the bit, add e and count; one butterfly per row.
//   k_rm1_weights  workgroup = user: m_u, w_uv = exp(L_uv - m_u) in place, B_u = sum_v w_uv beta_v.
//   k_rm1_score    workgroup = (tile of 8 users, chunk of columns).  A lane owns a column and walks its CSC entries in their stored
//                  order, one read of the entry serves the tile's eight accumulators; then p_i B_u, the log, m_u, -ln U_c, NaN on the
//                  user's own items, the (float) cast.  The rows go to the top-N kernels of the full job.
// All of it fp64, no floating-point atomics.  Every sum has a fixed order that depends on nothing but the data: a neighbour's row is
// summed by lane (entry index modulo 64) and a fixed butterfly, B_u by thread (v modulo 256) and a fixed tree, a column by one lane
// in stored order -- so a row's bits do not depend on the batch, the chunk widths, the tile it fell into or the entry point.
#include <algorithm>
#include <cmath>
#include <limits>

#include "fy_rm1.hpp"

namespace fy {
namespace {

constexpr int RM1_THREADS = 256;
constexpr int RM1_TILE = 8;                   // users that share a column read of k_rm1_score
constexpr int64_t RM1_LDS_MAX = 64 * 1024;    // bitmask bytes: 524 288 columns per cluster

__device__ __forceinline__ double rm1_neg_inf() { return __longlong_as_double(0xFFF0000000000000ll); }

__device__ __forceinline__ double rm1_wave_sum(double x) {      // every lane ends with the same bits (a + b = b + a at every level)
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ int rm1_wave_sum(int x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// p(i|C) and its log per (cluster, item) in rank order (k_req_p of the request path)
__global__ void k_rm1_p(int32_t nP, int32_t nI, const int32_t* __restrict__ rank_pair, const int32_t* __restrict__ pair_di,
                        const double* __restrict__ stats, double* __restrict__ p_rank, double* __restrict__ lnp_rank) {
    const double total = stats[nI] / 100.0;
    for (int32_t pos = blockIdx.x * blockDim.x + threadIdx.x; pos < nP; pos += gridDim.x * blockDim.x) {
        const double p = stats[pair_di[rank_pair[pos]]] / total;
        p_rank[pos] = p;
        lnp_rank[pos] = log(p);
    }
}

struct PrepArgs {
    int32_t s0, s1, pbase, general;
    double lambda;                            // Jelinek-Mercer: beta = lambda, w = 1 - lambda; general: beta_slot, w = 1
    const int32_t* __restrict__ rowptr;
    const int32_t* __restrict__ csr_idx;
    const float* __restrict__ csr_r;          // r' (the structure of an absolute-discounting job holds the discounted ratings)
    const double* __restrict__ usum_slot;     // d_v
    const double* __restrict__ beta_slot;
    const double* __restrict__ p_rank;
    const double* __restrict__ lnp_rank;
    double* __restrict__ e_csr;
    double* __restrict__ lp_slot;
    double* __restrict__ beta_out;
    double* __restrict__ lnbeta_out;
};

// one wave per user of the cluster: e_vj of its kept ratings, LP_v, beta_v, ln beta_v
__global__ __launch_bounds__(RM1_THREADS) void k_rm1_prep_rows(PrepArgs A) {
    const int lane = threadIdx.x & 63, wpb = RM1_THREADS >> 6;
    for (int32_t v = A.s0 + blockIdx.x * wpb + (threadIdx.x >> 6); v < A.s1; v += gridDim.x * wpb) {
        const double d = A.usum_slot[v];
        const double beta = A.general ? A.beta_slot[v] : A.lambda, w = A.general ? 1.0 : 1.0 - A.lambda;
        const int32_t f0 = A.rowptr[v], f1 = A.rowptr[v + 1];
        double lp = 0.0;
        for (int32_t f = f0 + lane; f < f1; f += 64) {
            const int32_t pos = A.pbase + A.csr_idx[f];
            const double lnp = A.lnp_rank[pos];
            const double c = w * ((double)A.csr_r[f] / d) + beta * A.p_rank[pos];
            A.e_csr[f] = log(c) - lnp;
            lp += lnp;
        }
        lp = rm1_wave_sum(lp);
        if (lane == 0) {
            A.lp_slot[v] = lp;
            A.beta_out[v] = beta;
            A.lnbeta_out[v] = log(beta);      // (beta = 0: -inf)
        }
    }
}

// a_vi = w r'_vi / d_v per CSC entry of the cluster
__global__ void k_rm1_prep_cols(int32_t q0, int32_t q1, double w, const int32_t* __restrict__ csc_slot, const float* __restrict__ csc_r,
                                const double* __restrict__ usum_slot, double* __restrict__ a_csc) {
    for (int64_t q = q0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < q1; q += (int64_t)gridDim.x * blockDim.x)
        a_csc[q] = w * ((double)csc_r[q] / usum_slot[csc_slot[q]]);
}

struct LoglikArgs {
    const int32_t* __restrict__ user_slot;    // [nb] slots of the batch's users
    int32_t Ic, s0, Uc, NCH, nvch, words;
    int64_t ldW;
    const int32_t* __restrict__ rowptr;
    const int32_t* __restrict__ csr_idx;
    const double* __restrict__ e_csr;
    const double* __restrict__ lp_slot;
    const double* __restrict__ lnbeta_slot;
    double* __restrict__ W;                   // [nb][ldW]: L_uv here, w_uv after k_rm1_weights
};

__global__ __launch_bounds__(RM1_THREADS) void k_rm1_loglik(LoglikArgs A) {
    extern __shared__ uint32_t rm1_mask[];    // [words]: bit i = the user rated column i
    const int32_t u = (int32_t)(blockIdx.x / (unsigned)A.nvch), ch = (int32_t)(blockIdx.x % (unsigned)A.nvch);
    const int32_t slot = A.user_slot[u];
    const int32_t f0 = A.rowptr[slot], f1 = A.rowptr[slot + 1], n_u = f1 - f0;
    for (int32_t t = threadIdx.x; t < A.words; t += RM1_THREADS) rm1_mask[t] = 0u;
    __syncthreads();
    for (int32_t f = f0 + (int32_t)threadIdx.x; f < f1; f += RM1_THREADS) {
        const int32_t j = A.csr_idx[f];
        if (j >= 0 && j < A.Ic) atomicOr(&rm1_mask[j >> 5], 1u << (j & 31));
    }
    __syncthreads();
    const double lp = A.lp_slot[slot];
    const int lane = threadIdx.x & 63;
    const int32_t v_end = min(A.Uc, (ch + 1) * A.NCH);
    double* __restrict__ out = A.W + (int64_t)u * A.ldW;
    for (int32_t vl = ch * A.NCH + (int32_t)(threadIdx.x >> 6); vl < v_end; vl += RM1_THREADS >> 6) {
        const int32_t v = A.s0 + vl;
        const int32_t g0 = A.rowptr[v], g1 = A.rowptr[v + 1];
        double E = 0.0;
        int cnt = 0;
        for (int32_t g = g0 + lane; g < g1; g += 64) {
            const int32_t j = A.csr_idx[g];
            if (j >= 0 && j < A.Ic && ((rm1_mask[j >> 5] >> (j & 31)) & 1u)) { E += A.e_csr[g]; cnt++; }
        }
        E = rm1_wave_sum(E);
        cnt = rm1_wave_sum(cnt);
        if (lane == 0) {
            double L = lp + E;
            if (cnt != n_u) L += (double)(n_u - cnt) * A.lnbeta_slot[v];      // (0 * -inf := 0)
            out[vl] = v == slot ? rm1_neg_inf() : L;
        }
    }
}

// one workgroup per user: m_u = max_v L_uv, w_uv = exp(L_uv - m_u) in place, B_u = sum_v w_uv beta_v (thread = v mod 256, fixed tree)
__global__ __launch_bounds__(RM1_THREADS) void k_rm1_weights(int32_t Uc, int32_t s0, int64_t ldW, const double* __restrict__ beta_slot,
                                                             double* __restrict__ W, double* __restrict__ m_out, double* __restrict__ B_out) {
    __shared__ double sh[RM1_THREADS];
    double* __restrict__ row = W + (int64_t)blockIdx.x * ldW;
    double m = rm1_neg_inf();
    for (int32_t vl = threadIdx.x; vl < Uc; vl += RM1_THREADS) m = fmax(m, row[vl]);
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int s = RM1_THREADS >> 1; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    m = sh[0];
    __syncthreads();
    const bool dead = !(m > rm1_neg_inf());      // no neighbour with a positive likelihood (or U_c = 1): every row is -inf
    double b = 0.0;
    for (int32_t vl = threadIdx.x; vl < Uc; vl += RM1_THREADS) {
        const double w = dead ? 0.0 : exp(row[vl] - m);
        row[vl] = w;
        b += w * beta_slot[s0 + vl];
    }
    sh[threadIdx.x] = b;
    __syncthreads();
    for (int s = RM1_THREADS >> 1; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) { m_out[blockIdx.x] = m; B_out[blockIdx.x] = sh[0]; }
}

struct ScoreRm1Args {
    const int32_t* __restrict__ user_slot;    // [nb]
    int32_t nb, Ic, s0, CCH, ncch, pbase;
    int64_t ldW, ldS;
    const int32_t* __restrict__ rank_pair;
    const int32_t* __restrict__ pair_start;
    const int32_t* __restrict__ csc_slot;
    const double* __restrict__ a_csc;
    const int32_t* __restrict__ rowptr;
    const int32_t* __restrict__ csr_idx;
    const double* __restrict__ p_rank;        // (+ pbase)
    const double* __restrict__ W;
    const double* __restrict__ m_u;
    const double* __restrict__ B_u;
    double ln_users;
    float* __restrict__ S;
};

__global__ __launch_bounds__(RM1_THREADS) void k_rm1_score(ScoreRm1Args A) {
    const int32_t tile = (int32_t)(blockIdx.x / (unsigned)A.ncch), ch = (int32_t)(blockIdx.x % (unsigned)A.ncch);
    const int32_t u0 = tile * RM1_TILE, nt = min(RM1_TILE, A.nb - u0);
    const double* __restrict__ wrow[RM1_TILE];
#pragma unroll
    for (int t = 0; t < RM1_TILE; t++) wrow[t] = A.W + (int64_t)(u0 + min(t, nt - 1)) * A.ldW;
    // (the last chunk also writes the padding of the rows: NaN, no candidate)
    const int64_t i_end = ch == A.ncch - 1 ? A.ldS : (int64_t)(ch + 1) * A.CCH;
    for (int64_t i = (int64_t)ch * A.CCH + threadIdx.x; i < i_end; i += RM1_THREADS) {
        const bool live = i < A.Ic;
        double acc[RM1_TILE];
#pragma unroll
        for (int t = 0; t < RM1_TILE; t++) acc[t] = 0.0;
        double p = 0.0;
        if (live) {
            const int32_t pr = A.rank_pair[A.pbase + i];
            const int32_t q0 = A.pair_start[pr], q1 = A.pair_start[pr + 1];
            for (int32_t q = q0; q < q1; q++) {      // the column's stored order
                const int32_t vl = A.csc_slot[q] - A.s0;
                const double a = A.a_csc[q];
#pragma unroll
                for (int t = 0; t < RM1_TILE; t++) acc[t] = fma(wrow[t][vl], a, acc[t]);
            }
            p = A.p_rank[i];
        }
#pragma unroll
        for (int t = 0; t < RM1_TILE; t++) {
            if (t < nt) {
                const int32_t slot = A.user_slot[u0 + t];
                int32_t lo = A.rowptr[slot], hi = A.rowptr[slot + 1];
                while (lo < hi) {      // is i one of the user's own items?  (a row's columns ascend)
                    const int32_t mid = (lo + hi) >> 1;
                    if ((int64_t)A.csr_idx[mid] < i) lo = mid + 1; else hi = mid;
                }
                const bool rated = live && lo < A.rowptr[slot + 1] && (int64_t)A.csr_idx[lo] == i;
                const double m = A.m_u[u0 + t];
                const double sc = m > rm1_neg_inf() ? (m - A.ln_users) + log(fma(p, A.B_u[u0 + t], acc[t])) : rm1_neg_inf();
                A.S[(int64_t)(u0 + t) * A.ldS + i] = live && !rated ? (float)sc : __uint_as_float(0x7FC00000u);
            }
        }
    }
}

struct Rm1User {
    int32_t slot, du, cluster, n_out, out_off;
};

}  // namespace

void rm1_score_slots(const RequestView& V, const std::vector<int32_t>& slots, fy_result* R) {
    Context* ctx = V.ctx;
    const Prepared& P = *V.P;
    const fy_rm2_params& prm = V.prm;
    hipStream_t st = ctx->stream;
    R->d_key0.alloc(ctx, 0);
    R->d_key1.alloc(ctx, 0);
    R->d_value.alloc(ctx, 0);
    R->d_aux.alloc(ctx, 0);
    if (P.nnz == 0 || slots.empty()) return;

    std::vector<std::vector<int32_t>> uploads;      // host sources of queued uploads live to the end of the call
    SyncOnUnwind drain(st);
    EventTimer t_tables(ctx), t_lik(ctx), t_score(ctx), t_topn(ctx);
    const size_t sp_tables = t_tables.begin();
    std::vector<int32_t> h_uid((size_t)P.nU), h_slot2du((size_t)P.nU), h_rowptr((size_t)P.nU + 1);
    d2h(ctx, h_uid.data(), P.uid.get(), (size_t)P.nU);
    d2h(ctx, h_slot2du.data(), P.slot2du.get(), (size_t)P.nU);
    d2h(ctx, h_rowptr.data(), P.rowptr.get(), (size_t)P.nU + 1);
    DevBuf<double> p_rank(ctx, (size_t)P.nP), lnp_rank(ctx, (size_t)P.nP);
    k_rm1_p<<<grid_for(P.nP), 256, 0, st>>>(P.nP, P.nI, P.rank_pair.get(), P.pair_di.get(), V.stats, p_rank.get(), lnp_rank.get());
    FY_KERNEL_CHECK();
    sync(ctx);

    // ---- per user: does it get a list, how long (k_user_meta of the full job)
    const int32_t N = prm.number_of_recommendations;
    std::vector<Rm1User> users;
    users.reserve(slots.size());
    std::vector<char> touched((size_t)P.K, 0);
    int64_t n_recs = 0, max_Ic = 0;
    {
        int c = 0;
        for (size_t k = 0; k < slots.size(); k++) {
            const int32_t slot = slots[k], du = h_slot2du[(size_t)slot];
            while (slot >= P.ucstart[c + 1]) c++;
            touched[(size_t)c] = 1;
            const int32_t Ic = P.pcstart[c + 1] - P.pcstart[c];
            const int32_t n = h_rowptr[(size_t)slot + 1] - h_rowptr[(size_t)slot];
            const int32_t unrated = Ic - n;
            if (unrated <= 0 || h_uid[(size_t)du] < prm.filter_users) continue;      // AbstractRM2Reducer.java:210-213, 221-223
            const int32_t keep = std::max(0, std::min(N, unrated));
            if (n_recs + keep > (int64_t)std::numeric_limits<int32_t>::max()) FY_FAIL(FY_ERR_UNSUPPORTED, "the result exceeds 2^31 rows");
            users.push_back(Rm1User{slot, du, c, keep, (int32_t)n_recs});
            n_recs += keep;
            max_Ic = std::max<int64_t>(max_Ic, Ic);
        }
    }
    for (int c = 0; c < P.K; c++) R->rq.clusters_touched += touched[(size_t)c];
    if (std::min<int64_t>(N, max_Ic) > TOPN_LIST_MAX)
        FY_FAIL(FY_ERR_UNSUPPORTED, "min(numberOfRecommendations, items per cluster) = %d exceeds the top-N kernel limit %d", (int)std::min<int64_t>(N, max_Ic), TOPN_LIST_MAX);
    R->n = n_recs;
    R->st.recs = n_recs;
    R->st.users_scored = (int64_t)users.size();
    R->d_key0.alloc(ctx, (size_t)n_recs);
    R->d_key1.alloc(ctx, (size_t)n_recs);
    R->d_value.alloc(ctx, (size_t)n_recs);
    R->d_aux.alloc(ctx, (size_t)n_recs);
    const size_t nus = users.size();
    if (nus == 0) {
        t_tables.end(sp_tables);
        sync(ctx);
        R->st.ms_tables = t_tables.total_ms();
        return;
    }
    DevBuf<int32_t> d_meta(ctx, 4 * nus);      // [slot][du][n_out][out_off] of the scored users
    {
        uploads.emplace_back(4 * nus);
        std::vector<int32_t>& h = uploads.back();
        for (size_t k = 0; k < nus; k++) {
            h[k] = users[k].slot; h[nus + k] = users[k].du; h[2 * nus + k] = users[k].n_out; h[3 * nus + k] = users[k].out_off;
        }
        h2d(ctx, d_meta.get(), h.data(), 4 * nus);
    }
    const int32_t *d_slot = d_meta.get(), *d_du = d_meta.get() + nus, *d_nout = d_meta.get() + 2 * nus, *d_off = d_meta.get() + 3 * nus;
    DevBuf<double> e_csr(ctx, (size_t)P.nnz), a_csc(ctx, (size_t)P.nnz), lp_slot(ctx, (size_t)P.nU), beta_slot(ctx, (size_t)P.nU),
        lnbeta_slot(ctx, (size_t)P.nU);
    t_tables.end(sp_tables);

    const int64_t ws = prm.workspace_bytes > 0 ? prm.workspace_bytes : ctx->tune.workspace_default;
    const double w_model = V.general ? 1.0 : 1.0 - prm.lambda;
    DevBuf<int32_t> overflow, any_overflow(ctx, 1);

    for (size_t k0 = 0; k0 < nus;) {
        const int c = users[k0].cluster;
        size_t k1 = k0;
        while (k1 < nus && users[k1].cluster == c) k1++;
        const int32_t Uc = P.csize[(size_t)c], Ic = P.pcstart[c + 1] - P.pcstart[c], pbase = P.pcstart[c], s0 = P.ucstart[c];
        const int64_t nnz_c = (int64_t)h_rowptr[(size_t)P.ucstart[c + 1]] - h_rowptr[(size_t)s0];
        const int32_t words = (int32_t)ceil_div(Ic, 32);
        if ((int64_t)words * 4 > RM1_LDS_MAX)
            FY_FAIL(FY_ERR_UNSUPPORTED, "RM1: cluster %d has %d items, the rated-set bitmask holds %lld", c, Ic, (long long)(RM1_LDS_MAX * 8));
        // ---- once per cluster: e, LP, beta, ln beta by row; a by column
        {
            const size_t sp = t_tables.begin();
            PrepArgs PA{s0, P.ucstart[c + 1], pbase, V.general ? 1 : 0, prm.lambda, P.rowptr.get(), P.csr_idx.get(), P.csr_r.get(), V.usum_slot,
                        V.general ? V.G.beta_slot : nullptr, p_rank.get(), lnp_rank.get(), e_csr.get(), lp_slot.get(), beta_slot.get(), lnbeta_slot.get()};
            k_rm1_prep_rows<<<grid_for((int64_t)Uc * 64, RM1_THREADS), RM1_THREADS, 0, st>>>(PA);
            FY_KERNEL_CHECK();
            const int32_t q0 = P.cluster_q[(size_t)c], q1 = P.cluster_q[(size_t)c + 1];
            k_rm1_prep_cols<<<grid_for(q1 - q0), 256, 0, st>>>(q0, q1, w_model, P.csc_slot.get(), P.csc_r.get(), V.usum_slot, a_csc.get());
            FY_KERNEL_CHECK();
            t_tables.end(sp);
        }
        const int64_t ldW = Uc, ldS = round_up(Ic, 256);
        const int64_t per_user = ldW * 8 + ldS * 4;
        const int64_t B = std::min<int64_t>((int64_t)(k1 - k0), ws / per_user);
        if (B < 1)
            FY_FAIL(FY_ERR_OUT_OF_MEMORY, "RM1: the weight and score rows of user %d alone (%lld bytes) exceed workspace_bytes = %lld",
                    h_uid[(size_t)users[k0].du], (long long)per_user, (long long)ws);
        const int32_t NCH = std::max(1, ctx->tune.rm1_nbr_chunk), nvch = (int32_t)ceil_div(Uc, NCH);
        const int32_t CCH = std::max(1, ctx->tune.rm1_col_chunk), ncch = (int32_t)ceil_div(Ic, CCH);
        if (B * nvch > 0x7FFFFFFFll || ceil_div(B, RM1_TILE) * ncch > 0x7FFFFFFFll)
            FY_FAIL(FY_ERR_UNSUPPORTED, "RM1: a batch of %lld users of cluster %d exceeds the launch grid", (long long)B, c);
        DevBuf<double> W(ctx, (size_t)(B * ldW)), m_u(ctx, (size_t)B), B_u(ctx, (size_t)B);
        DevBuf<float> Srows(ctx, (size_t)(B * ldS));
        if (overflow.size() < (size_t)B) overflow.alloc(ctx, (size_t)B);
        for (size_t b0 = k0; b0 < k1; b0 += (size_t)B) {
            const int32_t nb = (int32_t)std::min<size_t>((size_t)B, k1 - b0);
            R->rq.batches++;
            for (size_t k = b0; k < b0 + (size_t)nb; k++) {
                const int32_t n = h_rowptr[(size_t)users[k].slot + 1] - h_rowptr[(size_t)users[k].slot];
                R->st.pair_contribs += nnz_c - n;      // entries of the neighbours' rows tested against the user's bitmask
                R->st.log_terms += nnz_c;              // entries of the cluster's columns gathered for the user
            }
            const size_t sp_l = t_lik.begin();
            LoglikArgs LA{d_slot + b0, Ic, s0, Uc, NCH, nvch, words, ldW, P.rowptr.get(), P.csr_idx.get(), e_csr.get(), lp_slot.get(), lnbeta_slot.get(), W.get()};
            k_rm1_loglik<<<(unsigned)((int64_t)nb * nvch), RM1_THREADS, (size_t)words * 4, st>>>(LA);
            FY_KERNEL_CHECK();
            k_rm1_weights<<<(unsigned)nb, RM1_THREADS, 0, st>>>(Uc, s0, ldW, beta_slot.get(), W.get(), m_u.get(), B_u.get());
            FY_KERNEL_CHECK();
            t_lik.end(sp_l);
            R->st.cooc_launches++;
            const size_t sp_s = t_score.begin();
            ScoreRm1Args SA{d_slot + b0, nb, Ic, s0, CCH, ncch, pbase, ldW, ldS, P.rank_pair.get(), P.pair_start.get(), P.csc_slot.get(), a_csc.get(),
                            P.rowptr.get(), P.csr_idx.get(), p_rank.get() + pbase, W.get(), m_u.get(), B_u.get(), std::log((double)Uc), Srows.get()};
            k_rm1_score<<<(unsigned)(ceil_div(nb, RM1_TILE) * ncch), RM1_THREADS, 0, st>>>(SA);
            FY_KERNEL_CHECK();
            t_score.end(sp_s);
            R->st.score_launches++;
            const size_t sp_t = t_topn.begin();
            launch_topn_rows(ctx, st, Srows.get(), ldS, Ic, nb, d_nout + b0, d_off + b0, P.rank_item_raw.get() + pbase, d_du, P.uid.get(), (int32_t)b0, c,
                             R->d_key0.get(), R->d_key1.get(), R->d_value.get(), R->d_aux.get(), overflow.get(), any_overflow.get(), N);
            t_topn.end(sp_t);
        }
        k0 = k1;
    }
    sync(ctx);
    R->st.ms_tables = t_tables.total_ms();
    R->st.ms_cooc = t_lik.total_ms();
    R->st.ms_score = t_score.total_ms();
    R->st.ms_topn = t_topn.total_ms();
}

fy_result* rm1_score_users(const RequestView& V, const fy_rm2_request* rq) {
    Context* ctx = V.ctx;
    const Prepared& P = *V.P;
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
    EventTimer t_total(ctx);
    const size_t sp_total = t_total.begin();
    std::vector<int32_t> slots;
    if (P.nnz > 0 && rq->n_users > 0) {
        // the request: known users of this rank's share, once each, in the order of the unrestricted job (slot order)
        std::vector<int32_t> h_uid((size_t)P.nU), h_du2slot((size_t)P.nU);
        d2h(ctx, h_uid.data(), P.uid.get(), (size_t)P.nU);
        d2h(ctx, h_du2slot.data(), P.du2slot.get(), (size_t)P.nU);
        sync(ctx);
        slots.reserve((size_t)rq->n_users);
        for (int64_t t = 0; t < rq->n_users; t++) {
            const int32_t raw = rq->users[t];
            if (raw < 0) continue;
            auto it = std::lower_bound(h_uid.begin(), h_uid.end(), raw);
            if (it == h_uid.end() || *it != raw) continue;
            const int32_t slot = h_du2slot[(size_t)(it - h_uid.begin())];
            if (slot >= V.slot_lo && slot < V.slot_hi) slots.push_back(slot);
        }
        std::sort(slots.begin(), slots.end());
        slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    }
    R->rq.users_known = (int64_t)slots.size();
    rm1_score_slots(V, slots, R.get());
    t_total.end(sp_total);
    sync(ctx);
    R->st.ms_total = t_total.total_ms();
    return R.release();
}

}  // namespace fy
