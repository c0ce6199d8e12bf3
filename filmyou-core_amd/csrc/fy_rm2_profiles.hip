// fy_rm2_profiles.hip -- RM2 lists for GIVEN profiles and pending writes on a prepared job (fy_rm2_score_profiles).
//
// DESIGN.md section 2j.  A user's own rating VALUES never enter that user's scores, only the SET of rated items does (v != u leaves
// the own row out, s_u appears nowhere else).  With the cluster's statistics held as prepared, a composed profile therefore reads
// the slab rows G[j][.] of ITS items (k_req_slab of fy_rm2_request.hip, unchanged), masks ITS columns, and -- where the prepared row
// of the user holds a candidate i or an item j that the composition moved -- takes the user's own prepared products out of the sums:
//     term = (1-l)^2 (G[j][i] - x_uj x_ui) + q_j (b_i - x_ui) + a_i e_uj ,     x_u. = the PREPARED row (0 where it holds nothing).
// The ingest is sized by the request: T = the entries of this rank's profiles + (FY_PROFILE_ON_RESIDENT) the resident rows they go on.
//   k_rp_residents     label -> slot -> cluster, the length of the resident row (WHOLE: the given cluster, no row); unknown and
//                      filtered users get cluster -1 and their entries are not looked at
//   k_rp_keys          key = profile << cb | column over the T elements, resident elements IN FRONT of the given ones (raw item ->
//                      dense item -> (cluster, item) pair -> rank-order column; no column: the key of profile n, behind everything)
//   sort_pairs_u64_u32 stable: a run of one key keeps resident-then-given order, its last element counts
//   k_rp_runs          keep = last of its run, no delete, score > 0 (a resident element's score is); the counters
//   exclusive_scan_i32 place of every kept element
//   k_rp_rowptr        rowptr[p] = place of the first element whose key is >= p << cb
//   k_rp_scatter       the column and the PREPARED x_uj = r_uj / s_u of the resident row (0 for an item the row does not hold)
//   k_prof_score       one workgroup per (profile, 256 candidate columns), fp64: the composed row staged through LDS in blocks of
//                      256 as k_req_score stages the resident row; each lane finds its candidate's prepared x_ui once
// Where u is the ONLY rater of i or of j (pair_start) the own-term differences are exactly 0, and a remainder G - x_uj x_ui below what
// the slab resolves counts as 0: ln 0 = -inf at lambda = 0, as the full job gives.
// All stores are plain vector stores; the counters are a handful of wave-aggregated integer atomics; no floating-point atomics.
#include <algorithm>
#include <cmath>
#include <limits>

#include "fy_rm2_profiles.hpp"

namespace fy {
namespace {

enum { RC_USERS_UNKNOWN = 0, RC_USERS_FILTERED, RC_UNKNOWN_ITEM, RC_NONPOSITIVE, RC_SUPERSEDED, RC_REMOVES_HIT, RC_REMOVES_MISSED, RC_N };

constexpr int SCORE_COLS = 256;      // candidate columns of a scoring workgroup (one per lane)

inline int bits_for(int64_t v) {      // bits needed to hold the values 0 .. v
    int b = 1;
    while (b < 63 && (v >> b) != 0) b++;
    return b;
}

// the p in [0, n) with off[p] <= t < off[p + 1] (off ascending from 0, t < off[n])
__device__ __forceinline__ int32_t rp_owner(const int32_t* __restrict__ off, int32_t n, int32_t t) {
    return fy_lower_bound<true>(off, 0, n, t) - 1;
}

__device__ __forceinline__ void rp_count(unsigned long long* __restrict__ counters, int which, bool mine) {      // whole waves call it
    const unsigned long long b = __ballot(mine);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&counters[which], (unsigned long long)__popcll(b));
}

// the place of column col in the row [r0, r1) of csr_idx (ascending), -1 when the row does not hold it
__device__ __forceinline__ int32_t rp_find(const int32_t* __restrict__ csr_idx, int32_t r0, int32_t r1, int32_t col) {
    const int32_t lo = fy_lower_bound(csr_idx, r0, r1, col);
    return lo < r1 && csr_idx[lo] == col ? lo : -1;
}

struct ResidentArgs {
    int32_t n, resident;
    const int32_t* labels;
    const int32_t* cluster_in;      // FY_PROFILE_WHOLE
    const int32_t* uid;
    int32_t nU;
    const int32_t* du2slot;
    const int32_t* rowptr;
    const int32_t* ucstart;         // K + 1
    int32_t K, slot_lo, slot_hi, filter_users;
    int32_t* slot;                  // n: -1 = no resident row
    int32_t* pcl;                   // n: the cluster scored in, -1 = no list
    int32_t* rlen;                  // n + 1: length of the resident row; rlen[n] = 0
};

__global__ void k_rp_residents(ResidentArgs A, unsigned long long* __restrict__ counters) {
    const int64_t n_up = ((int64_t)A.n + 1 + 63) & ~(int64_t)63;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n_up; p += (int64_t)gridDim.x * blockDim.x) {
        bool unknown = false, filtered = false;
        if (p < A.n) {
            int32_t s = -1, c = -1, len = 0;
            if (A.resident) {
                const int32_t raw = A.labels[p];
                const int32_t lo = raw >= 0 ? fy_lower_bound(A.uid, 0, A.nU, raw) : A.nU;
                if (lo < A.nU && A.uid[lo] == raw) s = A.du2slot[lo];
                if (s < A.slot_lo || s >= A.slot_hi) s = -1;
                unknown = s < 0;
                filtered = !unknown && raw < A.filter_users;
                if (filtered) s = -1;
                if (s >= 0) {
                    c = fy_lower_bound<true>(A.ucstart, 0, A.K + 1, s) - 1;
                    len = A.rowptr[s + 1] - A.rowptr[s];
                }
            } else {
                c = A.cluster_in[p];
            }
            A.slot[p] = s;
            A.pcl[p] = c;
            A.rlen[p] = len;
        } else if (p == A.n) {
            A.rlen[p] = 0;
        }
        rp_count(counters, RC_USERS_UNKNOWN, unknown);
        rp_count(counters, RC_USERS_FILTERED, filtered);
    }
}

struct ProfIn {
    int32_t n;                      // profiles of this rank
    int32_t T, Rn;                  // elements, of which the first Rn are resident elements
    int cb;                         // bits of a column
    const int32_t* roff;            // n + 1: first resident element of every profile (Rn > 0)
    const int32_t* slot;            // n
    const int32_t* pcl;             // n
    const int32_t* start;           // n + 1: first given entry of every profile, from 0
    const int32_t* item;            // T - Rn given entries
    const float* score;
    const uint8_t* remove;          // or nullptr
    const int32_t* rowptr;          // the job's CSR
    const int32_t* csr_idx;
    const float* csr_r;
    const double* usum_slot;
    const int32_t* iid;             // raw ids of the nI dense items, ascending
    int32_t nI;
    const int32_t* pcstart;         // K + 1: the pairs / the rank-order positions of every cluster
    const int32_t* pair_di;         // dense item of every pair, ascending inside a cluster
    const int32_t* pair_rank;       // rank-order column of every pair inside its cluster
};

__global__ void k_rp_keys(ProfIn A, uint64_t* __restrict__ keys, uint32_t* __restrict__ pos, unsigned long long* __restrict__ counters) {
    const int64_t t_up = ((int64_t)A.T + 63) & ~(int64_t)63;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < t_up; t += (int64_t)gridDim.x * blockDim.x) {
        bool no_column = false;
        if (t < A.T) {
            int32_t p, col = -1;
            if (t < A.Rn) {
                p = rp_owner(A.roff, A.n, (int32_t)t);
                col = A.csr_idx[A.rowptr[A.slot[p]] + ((int32_t)t - A.roff[p])];
            } else {
                const int32_t e = (int32_t)t - A.Rn;
                p = rp_owner(A.start, A.n, e);
                const int32_t c = A.pcl[p];
                if (c >= 0) {      // (the entries of a profile without a list are not looked at)
                    const int32_t raw = A.item[e];
                    const int32_t di = raw >= 0 ? fy_lower_bound(A.iid, 0, A.nI, raw) : A.nI;
                    if (di < A.nI && A.iid[di] == raw) {
                        const int32_t q0 = A.pcstart[c], q1 = A.pcstart[c + 1];
                        const int32_t pr = fy_lower_bound(A.pair_di, q0, q1, di);
                        if (pr < q1 && A.pair_di[pr] == di) col = A.pair_rank[pr];
                    }
                    no_column = col < 0;
                }
            }
            keys[t] = col < 0 ? ((uint64_t)(uint32_t)A.n << A.cb) : (((uint64_t)(uint32_t)p << A.cb) | (uint32_t)col);
            pos[t] = (uint32_t)t;
        }
        rp_count(counters, RC_UNKNOWN_ITEM, no_column);
    }
}

// keep[x] (x <= T; keep[T] = 0): sorted element x is the last of its key's run, belongs to a profile, is no delete and has score > 0
__global__ void k_rp_runs(ProfIn A, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ spos, int32_t* __restrict__ keep,
                          unsigned long long* __restrict__ counters) {
    const int64_t t_up = ((int64_t)A.T + 1 + 63) & ~(int64_t)63;
    const uint64_t col_mask = ((uint64_t)1 << A.cb) - 1;
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < t_up; x += (int64_t)gridDim.x * blockDim.x) {
        int kind = -1;      // 0 superseded, 1 a delete that hit the resident row, 2 a delete that missed, 3 a score that is not > 0
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
                    const int32_t s = A.slot[p];
                    kind = s >= 0 && rp_find(A.csr_idx, A.rowptr[s], A.rowptr[s + 1], (int32_t)(key & col_mask)) >= 0 ? 1 : 2;
                } else if (given && !(A.score[t - A.Rn] > 0.0f)) {
                    kind = 3;
                } else {
                    k = true;
                }
            }
        }
        if (x <= A.T) keep[x] = k;
        rp_count(counters, RC_SUPERSEDED, kind == 0);
        rp_count(counters, RC_REMOVES_HIT, kind == 1);
        rp_count(counters, RC_REMOVES_MISSED, kind == 2);
        rp_count(counters, RC_NONPOSITIVE, kind == 3);
    }
}

// rowptr[p], p <= n: the place of the first kept element of profile p (place[T] = all kept elements)
__global__ void k_rp_rowptr(int32_t n, int32_t T, int cb, const uint64_t* __restrict__ skeys, const int32_t* __restrict__ place,
                            int32_t* __restrict__ rowptr) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p <= n; p += (int64_t)gridDim.x * blockDim.x)
        rowptr[p] = place[fy_lower_bound(skeys, 0, T, (uint64_t)p << cb)];
}

__global__ void k_rp_scatter(ProfIn A, const uint64_t* __restrict__ skeys, const int32_t* __restrict__ keep, const int32_t* __restrict__ place,
                             int32_t* __restrict__ o_idx, double* __restrict__ o_x) {
    const uint64_t col_mask = ((uint64_t)1 << A.cb) - 1;
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < A.T; x += (int64_t)gridDim.x * blockDim.x) {
        if (!keep[x]) continue;
        const uint64_t key = skeys[x];
        const int32_t col = (int32_t)(key & col_mask), at = place[x];
        const int32_t s = A.slot[(int32_t)(key >> A.cb)];
        double xp = 0.0;      // the PREPARED weight, whatever score the kept element carries: only the set of items enters
        if (s >= 0) {
            const int32_t f = rp_find(A.csr_idx, A.rowptr[s], A.rowptr[s + 1], col);
            if (f >= 0) xp = (double)A.csr_r[f] / A.usum_slot[s];
        }
        o_idx[at] = col;
        o_x[at] = xp;
    }
}

struct ProfScoreArgs {
    const int32_t* __restrict__ prof;       // [nb] profiles of the batch (positions in this rank's range)
    const int32_t* __restrict__ c_rowptr;   // the composed rows
    const int32_t* __restrict__ c_idx;
    const double* __restrict__ c_x;
    const int32_t* __restrict__ slot;       // by profile: the resident row (-1: none)
    const int32_t* __restrict__ slotmap;    // [Ic] item index -> slab row
    const double* __restrict__ slab;
    int64_t ld;
    int32_t Ic, n_chunks;
    const int32_t* __restrict__ rowptr;
    const int32_t* __restrict__ csr_idx;
    const float* __restrict__ csr_r;
    const double* __restrict__ usum_slot;
    const double* __restrict__ p_rank;      // (+ pbase)
    const double* __restrict__ b_rank;      // (+ pbase)
    const int32_t* __restrict__ rank_pair;  // (+ pbase)
    const int32_t* __restrict__ pair_start;
    double lambda, ln_items, ln_users, n_others;
    float* __restrict__ S;
    int64_t ldS;
};

__global__ __launch_bounds__(SCORE_COLS) void k_prof_score(ProfScoreArgs A) {
    __shared__ double sh_e[SCORE_COLS], sh_e0[SCORE_COLS], sh_q[SCORE_COLS], sh_x[SCORE_COLS], sh_res[SCORE_COLS];
    __shared__ int32_t sh_row[SCORE_COLS], sh_j[SCORE_COLS], sh_only[SCORE_COLS];
    const int32_t u = (int32_t)(blockIdx.x / (unsigned)A.n_chunks), ch = (int32_t)(blockIdx.x % (unsigned)A.n_chunks);
    const int32_t i = ch * SCORE_COLS + (int32_t)threadIdx.x;
    const int32_t p = A.prof[u];
    const int32_t f0 = A.c_rowptr[p], f1 = A.c_rowptr[p + 1];
    const int32_t slot = A.slot[p];
    const bool live = i < A.Ic;
    const double a_i = live ? A.lambda * A.p_rank[i] : 0.0;
    double b_i = live ? A.b_rank[i] : 0.0;
    const double w2 = (1.0 - A.lambda) * (1.0 - A.lambda), w1 = A.lambda * (1.0 - A.lambda);
    // the candidate's prepared x_ui: not 0 only for an item of the resident row that the profile no longer holds
    bool own_i = false, only_i = false;
    double x_i = 0.0;
    if (live && slot >= 0) {
        const int32_t f = rp_find(A.csr_idx, A.rowptr[slot], A.rowptr[slot + 1], i);
        if (f >= 0) {
            own_i = true;
            x_i = (double)A.csr_r[f] / A.usum_slot[slot];
            const int32_t pr = A.rank_pair[i];
            only_i = A.pair_start[pr + 1] - A.pair_start[pr] == 1;
            b_i = only_i ? 0.0 : b_i - x_i;      // sum over v != u of x_vi; u alone rated i: exactly 0
            if (!(b_i > 0.0)) b_i = 0.0;
        }
    }
    double acc = 0.0;
    bool rated = false;
    for (int32_t base = f0; base < f1; base += SCORE_COLS) {       // (block-uniform)
        const int32_t f = base + (int32_t)threadIdx.x;
        if (f < f1) {
            const int32_t j = A.c_idx[f];
            const double x = A.c_x[f];
            const double pj = A.p_rank[j];
            const int32_t pr = A.rank_pair[j];
            const int32_t raters = A.pair_start[pr + 1] - A.pair_start[pr];
            const bool only_j = x > 0.0 && raters == 1;
            const double b_j = A.b_rank[j];
            const double e = fy_req_e(A.lambda, b_j, x, A.n_others, pj);
            sh_e[threadIdx.x] = e;                                                         // what k_req_score forms: candidates the row never held
            sh_e0[threadIdx.x] = only_j ? fy_req_e(A.lambda, x, x, A.n_others, pj) : e;    // u the only rater of j: b_j - x_uj is exactly 0
            sh_q[threadIdx.x] = w1 * pj;
            sh_x[threadIdx.x] = x;
            sh_j[threadIdx.x] = j;
            sh_row[threadIdx.x] = A.slotmap[j];
            sh_only[threadIdx.x] = only_j;
            // what the slab's row j resolves: every one of its contributions was rounded to 2^(ex - 61) (k_req_slab)
            sh_res[threadIdx.x] = ldexp((double)raters, max(-900, min(ilogb(b_j), 60)) - 61);
        }
        __syncthreads();
        const int32_t m = min(SCORE_COLS, f1 - base);
        if (live)
            for (int32_t k = 0; k < m; k++) {
                rated |= sh_j[k] == i;
                const int32_t r = sh_row[k];
                double g = r >= 0 ? A.slab[(int64_t)r * A.ld + i] : __longlong_as_double(0x7FF8000000000000ll);
                double e = sh_e[k];
                if (own_i) {      // the user's own product leaves the sum; u the only rater of i or of j: exactly 0
                    const double noise = sh_res[k] + g * 0x1p-51;      // a remainder the slab's fixed point and its fp64 rounding cannot tell from 0
                    g = only_i || sh_only[k] ? 0.0 : g - sh_x[k] * x_i;
                    if (!(g > noise)) g = 0.0;
                    e = sh_e0[k];
                }
                acc += fy_req_log_term(w2, g, sh_q[k], b_i, a_i, e);
            }
        __syncthreads();
    }
    A.S[(int64_t)u * A.ldS + i] = live && !rated ? fy_req_row_value(acc, (double)(f1 - f0), A.ln_items, A.ln_users) : __uint_as_float(0x7FC00000u);
}

struct PlanProfile {
    int32_t p, cluster, n_out, out_off;
};

}  // namespace

fy_result* rm2_score_profiles(fy_rm2_job* J, const fy_rm2_profiles* pf) {
    // ---- what the host refuses before any launch
    fy_rm2_params jp{};
    bool have_coll = false;
    rm2_job_peek(J, &jp, &have_coll);
    if (jp.flags & FY_RM2_ESTIMATOR_RM1) FY_FAIL(FY_ERR_UNSUPPORTED, "fy_rm2_score_profiles: the job runs the RM1 estimator");
    if (smoothing_of(jp).general())
        FY_FAIL(FY_ERR_UNSUPPORTED, "fy_rm2_score_profiles: Dirichlet-prior and absolute-discounting jobs are not served (Jelinek-Mercer only)");
    if (have_coll) FY_FAIL(FY_ERR_UNSUPPORTED, "fy_rm2_score_profiles: the job has collectives installed (the cooperative path serves no requests)");
    if (jp.world != 1) FY_FAIL(FY_ERR_UNSUPPORTED, "fy_rm2_score_profiles: the job was prepared with world = %d; profiles are served by a one-rank job", jp.world);
    if (pf->n_profiles < 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "n_profiles < 0");
    if (pf->base != FY_PROFILE_WHOLE && pf->base != FY_PROFILE_ON_RESIDENT) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "base %d is neither FY_PROFILE_WHOLE nor FY_PROFILE_ON_RESIDENT", pf->base);
    if (pf->world < 1 || pf->rank < 0 || pf->rank >= pf->world) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "rank %d of world %d", pf->rank, pf->world);
    const int64_t n_all = pf->n_profiles;
    const bool resident = pf->base == FY_PROFILE_ON_RESIDENT;
    if (n_all > 0) {
        if (!pf->user || !pf->start) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "user or start is NULL");
        if (pf->start[0] != 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "start[0] is %lld: the offsets begin at 0", (long long)pf->start[0]);
        for (int64_t p = 0; p < n_all; p++)
            if (pf->start[p + 1] < pf->start[p]) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "start decreases at profile %lld", (long long)p);
        if (pf->start[n_all] > 0 && (!pf->item || !pf->score)) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "item or score is NULL");
        if (!resident && !pf->cluster) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "FY_PROFILE_WHOLE needs the cluster of every profile: cluster is NULL");
        if (pf->start[n_all] > (int64_t)std::numeric_limits<int32_t>::max())
            FY_FAIL(FY_ERR_UNSUPPORTED, "%lld profile entries: at most 2^31 - 1", (long long)pf->start[n_all]);
    }
    if (n_all > (int64_t)std::numeric_limits<int32_t>::max()) FY_FAIL(FY_ERR_UNSUPPORTED, "%lld profiles: at most 2^31 - 1", (long long)n_all);

    RequestView V;
    rm2_request_view(J, V);
    Context* ctx = V.ctx;
    const Prepared& P = *V.P;
    const fy_rm2_params& prm = V.prm;
    if (!resident)
        for (int64_t p = 0; p < n_all; p++) {
            const int32_t c = pf->cluster[p];
            if (c < 0 || c >= prm.number_of_clusters || c >= P.K) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "cluster[%lld] = %d is outside [0, %d)", (long long)p, c, prm.number_of_clusters);
            if (P.nnz > 0 && P.csize[(size_t)c] == 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "cluster[%lld] = %d names an empty cluster", (long long)p, c);
        }
    hipStream_t st = ctx->stream;
    std::unique_ptr<fy_result> R(new fy_result);
    R->ctx = ctx;
    R->kind = 0;
    R->has_rm2_profile_stats = true;
    fy_rm2_profile_stats& ps = R->rpf;
    ps.profiles_asked = n_all;
    R->st.nnz = P.nnz;
    R->st.n_users = P.nU;
    R->st.n_items = P.nI;
    R->d_user_id.alloc(ctx, 0);
    R->d_item_id.alloc(ctx, 0);
    if (P.nnz == 0 || n_all == 0) return R.release();

    // ---- this rank's profiles: a contiguous range of the list given
    const int64_t plo = n_all * pf->rank / pf->world, phi = n_all * (pf->rank + 1) / pf->world;
    const int32_t n = (int32_t)(phi - plo);
    const int64_t e0 = pf->start[plo];
    const int32_t E = (int32_t)(pf->start[phi] - e0);
    ps.profiles_mine = n;
    ps.entries = E;
    if (n == 0) return R.release();

    std::vector<int32_t> h_start((size_t)n + 1);
    for (int32_t p = 0; p <= n; p++) h_start[(size_t)p] = (int32_t)(pf->start[plo + p] - e0);
    unsigned long long h_c[RC_N] = {};
    std::vector<std::vector<int32_t>> uploads;      // host buffers of queued uploads live to the end of the call
    SyncOnUnwind drain(st);                         // a failure drains the stream before they (and the caller's arrays) go
    EventTimer t_total(ctx), t_tables(ctx), t_cooc(ctx), t_score(ctx), t_topn(ctx);
    const size_t sp_total = t_total.begin();
    const size_t sp_tables = t_tables.begin();
    RequestState& S = rm2_request_state(V);
    DevBuf<double> p_rank(ctx, (size_t)P.nP);
    rm2_request_p(V, p_rank.get());

    // ---- the profiles in HBM
    DevBuf<int32_t> labels(ctx, (size_t)n), start(ctx, (size_t)n + 1), item(ctx, (size_t)E), cluster_in;
    DevBuf<float> score(ctx, (size_t)E);
    DevBuf<uint8_t> remove;
    DevBuf<unsigned long long> counters(ctx, RC_N);
    counters.zero();
    h2d(ctx, labels.get(), pf->user + plo, (size_t)n);
    h2d(ctx, start.get(), h_start.data(), (size_t)n + 1);
    h2d(ctx, item.get(), pf->item + e0, (size_t)E);
    h2d(ctx, score.get(), pf->score + e0, (size_t)E);
    if (pf->remove && E > 0) {
        remove.alloc(ctx, (size_t)E);
        h2d(ctx, remove.get(), pf->remove + e0, (size_t)E);
    }
    if (!resident) {
        cluster_in.alloc(ctx, (size_t)n);
        h2d(ctx, cluster_in.get(), pf->cluster + plo, (size_t)n);
    }
    // ---- slot, cluster and resident row of every profile
    DevBuf<int32_t> slot(ctx, (size_t)n), pcl(ctx, (size_t)n), rlen(ctx, (size_t)n + 1), roff(ctx, (size_t)n + 1);
    {
        ResidentArgs A{};
        A.n = n; A.resident = resident ? 1 : 0;
        A.labels = labels.get(); A.cluster_in = cluster_in.get();
        A.uid = P.uid.get(); A.nU = P.nU; A.du2slot = P.du2slot.get(); A.rowptr = P.rowptr.get(); A.ucstart = P.d_ucstart.get();
        A.K = P.K; A.slot_lo = V.slot_lo; A.slot_hi = V.slot_hi; A.filter_users = prm.filter_users;
        A.slot = slot.get(); A.pcl = pcl.get(); A.rlen = rlen.get();
        k_rp_residents<<<grid_for((int64_t)n + 1), 256, 0, st>>>(A, counters.get());
        FY_KERNEL_CHECK();
    }
    std::vector<int32_t> h_slot((size_t)n), h_pcl((size_t)n), h_rlen((size_t)n);
    d2h(ctx, h_slot.data(), slot.get(), (size_t)n);
    d2h(ctx, h_pcl.data(), pcl.get(), (size_t)n);
    d2h(ctx, h_rlen.data(), rlen.get(), (size_t)n);
    exclusive_scan_i32(ctx, rlen.get(), roff.get(), (size_t)n + 1);
    sync(ctx);
    int64_t Rn = 0;
    for (int32_t v : h_rlen) Rn += v;
    if (Rn + E > (int64_t)std::numeric_limits<int32_t>::max())
        FY_FAIL(FY_ERR_UNSUPPORTED, "%lld resident elements + %lld entries: a request composes at most 2^31 - 1 elements", (long long)Rn, (long long)E);
    const int32_t T = (int32_t)(Rn + E);

    // ---- compose: keys, stable sort, last of every run, scan, scatter
    int64_t max_Ic_all = 1;
    for (int c = 0; c < P.K; c++) max_Ic_all = std::max<int64_t>(max_Ic_all, P.pcstart[c + 1] - P.pcstart[c]);
    DevBuf<int32_t> c_rowptr(ctx, (size_t)n + 1), c_idx(ctx, (size_t)T);
    DevBuf<double> c_x(ctx, (size_t)T);
    std::vector<int32_t> h_rowptr((size_t)n + 1, 0), h_idx;
    if (T > 0) {
        ProfIn A{};
        A.n = n; A.T = T; A.Rn = (int32_t)Rn;
        A.cb = bits_for(max_Ic_all - 1);
        A.roff = roff.get(); A.slot = slot.get(); A.pcl = pcl.get(); A.start = start.get();
        A.item = item.get(); A.score = score.get(); A.remove = remove.get();
        A.rowptr = P.rowptr.get(); A.csr_idx = P.csr_idx.get(); A.csr_r = P.csr_r.get(); A.usum_slot = V.usum_slot;
        A.iid = P.iid.get(); A.nI = P.nI; A.pcstart = P.d_pcstart.get(); A.pair_di = P.pair_di.get(); A.pair_rank = P.pair_rank.get();
        DevBuf<uint64_t> keys(ctx, (size_t)T), skeys(ctx, (size_t)T);
        DevBuf<uint32_t> pos(ctx, (size_t)T), spos(ctx, (size_t)T);
        DevBuf<int32_t> keep(ctx, (size_t)T + 1), place(ctx, (size_t)T + 1);
        k_rp_keys<<<grid_for(T), 256, 0, st>>>(A, keys.get(), pos.get(), counters.get());
        FY_KERNEL_CHECK();
        sort_pairs_u64_u32(ctx, keys.get(), skeys.get(), pos.get(), spos.get(), (size_t)T, A.cb + bits_for(n));      // stable
        k_rp_runs<<<grid_for((int64_t)T + 1), 256, 0, st>>>(A, skeys.get(), spos.get(), keep.get(), counters.get());
        FY_KERNEL_CHECK();
        exclusive_scan_i32(ctx, keep.get(), place.get(), (size_t)T + 1);
        k_rp_rowptr<<<grid_for((int64_t)n + 1), 256, 0, st>>>(n, T, A.cb, skeys.get(), place.get(), c_rowptr.get());
        FY_KERNEL_CHECK();
        k_rp_scatter<<<grid_for(T), 256, 0, st>>>(A, skeys.get(), keep.get(), place.get(), c_idx.get(), c_x.get());
        FY_KERNEL_CHECK();
        d2h(ctx, h_rowptr.data(), c_rowptr.get(), (size_t)n + 1);
        d2h(ctx, h_c, counters.get(), RC_N);
        sync(ctx);
        const int32_t composed = h_rowptr[(size_t)n];
        if (composed < 0 || composed > T) FY_FAIL(FY_ERR_HIP, "profiles: %d composed items of %d elements", composed, T);
        h_idx.resize((size_t)composed);
        d2h(ctx, h_idx.data(), c_idx.get(), (size_t)composed);
        sync(ctx);
    } else {
        d2h(ctx, h_c, counters.get(), RC_N);
        sync(ctx);
    }
    ps.users_unknown = (int64_t)h_c[RC_USERS_UNKNOWN];
    ps.users_filtered = (int64_t)h_c[RC_USERS_FILTERED];
    ps.entries_unknown_item = (int64_t)h_c[RC_UNKNOWN_ITEM];
    ps.entries_nonpositive = (int64_t)h_c[RC_NONPOSITIVE];
    ps.entries_superseded = (int64_t)h_c[RC_SUPERSEDED];
    ps.removes_hit = (int64_t)h_c[RC_REMOVES_HIT];
    ps.removes_missed = (int64_t)h_c[RC_REMOVES_MISSED];
    ps.items_composed = h_rowptr[(size_t)n];

    // ---- the plan: which profile gets a list and how long; rows come out in the order given, the work goes cluster by cluster
    const int32_t N = prm.number_of_recommendations;
    std::vector<PlanProfile> plan;
    int64_t n_recs = 0, log_terms = 0, max_Ic = 0;
    for (int32_t p = 0; p < n; p++) {
        const int32_t c = h_pcl[(size_t)p];
        if (c < 0) continue;
        const int32_t np = h_rowptr[(size_t)p + 1] - h_rowptr[(size_t)p];
        if (np == 0) { ps.profiles_empty++; continue; }
        const int32_t Ic = P.pcstart[c + 1] - P.pcstart[c], unrated = Ic - np;
        if (unrated <= 0) continue;
        const int32_t keep = std::max(0, std::min(N, unrated));
        if (n_recs + keep > (int64_t)std::numeric_limits<int32_t>::max()) FY_FAIL(FY_ERR_UNSUPPORTED, "the request's result exceeds 2^31 rows");
        plan.push_back(PlanProfile{p, c, keep, (int32_t)n_recs});
        ps.profiles_scored += keep > 0;
        n_recs += keep;
        log_terms += (int64_t)np * unrated;
        max_Ic = std::max<int64_t>(max_Ic, Ic);
    }
    if (std::min<int64_t>(N, max_Ic) > TOPN_LIST_MAX)
        FY_FAIL(FY_ERR_UNSUPPORTED, "min(numberOfRecommendations, items per cluster) = %d exceeds the top-N kernel limit %d", (int)std::min<int64_t>(N, max_Ic), TOPN_LIST_MAX);
    std::stable_sort(plan.begin(), plan.end(), [](const PlanProfile& a, const PlanProfile& b) { return a.cluster < b.cluster; });
    R->n = n_recs;
    R->st.recs = n_recs;
    R->st.users_scored = ps.profiles_scored;
    R->st.log_terms = log_terms;
    R->d_key0.alloc(ctx, (size_t)n_recs);
    R->d_key1.alloc(ctx, (size_t)n_recs);
    R->d_value.alloc(ctx, (size_t)n_recs);
    R->d_aux.alloc(ctx, (size_t)n_recs);
    const size_t nus = plan.size();
    DevBuf<int32_t> d_meta(ctx, 3 * nus + 3);      // [profile][n_out][out_off] of the planned profiles, cluster by cluster
    if (nus) {
        uploads.emplace_back(3 * nus);
        std::vector<int32_t>& h = uploads.back();
        for (size_t k = 0; k < nus; k++) { h[k] = plan[k].p; h[nus + k] = plan[k].n_out; h[2 * nus + k] = plan[k].out_off; }
        h2d(ctx, d_meta.get(), h.data(), 3 * nus);
    }
    const int32_t *d_prof = d_meta.get(), *d_nout = d_meta.get() + nus, *d_off = d_meta.get() + 2 * nus;
    t_tables.end(sp_tables);

    const int64_t ws = prm.workspace_bytes > 0 ? prm.workspace_bytes : ctx->tune.workspace_default;
    const double lambda = prm.lambda;
    std::vector<int32_t> stamp;            // item index -> slab row of the batch being planned (-1: none)
    DevBuf<int32_t> overflow, any_overflow(ctx, 1);
    for (size_t k0 = 0; k0 < nus;) {
        const int c = plan[k0].cluster;
        size_t k1 = k0;
        while (k1 < nus && plan[k1].cluster == c) k1++;
        ps.clusters_touched++;
        const int32_t Uc = P.csize[(size_t)c], Ic = P.pcstart[c + 1] - P.pcstart[c], pbase = P.pcstart[c];
        const int64_t ld = round_up(Ic, 32), ldS = round_up(Ic, SCORE_COLS);
        const int32_t CH = (int32_t)std::min<int64_t>(S.CH, round_up(Ic, 64)), nch = (int32_t)ceil_div(Ic, CH);
        const int64_t max_rows = ws / (ld * 8);
        // ---- batches of profiles whose union J fits the slab
        for (size_t b0 = k0; b0 < k1;) {
            stamp.assign((size_t)Ic, -1);
            std::vector<int32_t> rows;
            size_t b1 = b0;
            for (; b1 < k1; b1++) {
                const int32_t p = plan[b1].p;
                const int32_t f0 = h_rowptr[(size_t)p], f1 = h_rowptr[(size_t)p + 1];
                int64_t fresh_rows = 0;
                for (int32_t f = f0; f < f1; f++) fresh_rows += stamp[(size_t)h_idx[(size_t)f]] < 0;
                if ((int64_t)rows.size() + fresh_rows > max_rows) {
                    if (b1 == b0)
                        FY_FAIL(FY_ERR_OUT_OF_MEMORY, "fy_rm2_score_profiles: the %lld matrix rows of profile %lld (label %d) alone (%lld bytes) exceed workspace_bytes = %lld",
                                (long long)fresh_rows, (long long)(plo + p), pf->user[plo + p], (long long)(fresh_rows * ld * 8), (long long)ws);
                    break;
                }
                for (int32_t f = f0; f < f1; f++) {
                    const int32_t j = h_idx[(size_t)f];
                    if (stamp[(size_t)j] < 0) { stamp[(size_t)j] = (int32_t)rows.size(); rows.push_back(j); }
                }
            }
            const int32_t nJ = (int32_t)rows.size(), nb_all = (int32_t)(b1 - b0);
            ps.batches++;
            ps.slab_rows += nJ;
            ps.slab_bytes_peak = std::max<int64_t>(ps.slab_bytes_peak, (int64_t)nJ * ld * 8);
            for (int32_t j : rows) ps.slab_pair_contribs += S.walk[(size_t)pbase + (size_t)j];
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
                        S.choff.get(), P.csr_idx.get(), P.csr_r.get(), V.usum_slot, V.b_rank, slab.get(), nullptr, 0.0};
            rm2_launch_req_slab(st, SA, "fy_rm2_score_profiles");
            t_cooc.end(sp_c);
            R->st.cooc_launches++;
            // ---- scoring + top-N in groups of profiles whose float rows fit 256 MB
            const int32_t G = (int32_t)std::max<int64_t>(1, std::min<int64_t>(nb_all, ((int64_t)256 << 20) / (ldS * 4)));
            DevBuf<float> Srows(ctx, (size_t)G * (size_t)ldS);
            if (overflow.size() < (size_t)G) overflow.alloc(ctx, (size_t)G);
            const int32_t n_chunks = (int32_t)(ldS / SCORE_COLS);
            const int32_t n_nb = resident ? Uc : Uc + 1;      // the cluster as the profile sees it: WHOLE is its (U_c + 1)-th member
            for (int32_t g0 = 0; g0 < nb_all; g0 += G) {
                const int32_t nb = std::min(G, nb_all - g0);
                const size_t first = b0 + (size_t)g0;
                const size_t sp_s = t_score.begin();
                ProfScoreArgs A{d_prof + first, c_rowptr.get(), c_idx.get(), c_x.get(), slot.get(), d_plan.get() + nJ, slab.get(), ld, Ic, n_chunks,
                                P.rowptr.get(), P.csr_idx.get(), P.csr_r.get(), V.usum_slot, p_rank.get() + pbase, V.b_rank + pbase,
                                P.rank_pair.get() + pbase, P.pair_start.get(), lambda, std::log((double)prm.number_of_items), std::log((double)n_nb),
                                (double)(n_nb - 1), Srows.get(), ldS};
                k_prof_score<<<(unsigned)((int64_t)nb * n_chunks), SCORE_COLS, 0, st>>>(A);
                FY_KERNEL_CHECK();
                t_score.end(sp_s);
                R->st.score_launches++;
                const size_t sp_t = t_topn.begin();
                // (the labels stand where the user ids do: row u of the batch is named labels[prof[first + u]])
                launch_topn_rows(ctx, st, Srows.get(), ldS, Ic, nb, d_nout + first, d_off + first, P.rank_item_raw.get() + pbase, d_prof, labels.get(),
                                 (int32_t)first, c, R->d_key0.get(), R->d_key1.get(), R->d_value.get(), R->d_aux.get(), overflow.get(),
                                 any_overflow.get(), N);
                t_topn.end(sp_t);
            }
            b0 = b1;
        }
        k0 = k1;
    }
    t_total.end(sp_total);
    sync(ctx);
    R->st.pair_contribs = ps.slab_pair_contribs;
    R->st.ms_tables = t_tables.total_ms();
    R->st.ms_cooc = t_cooc.total_ms();
    R->st.ms_score = t_score.total_ms();
    R->st.ms_topn = t_topn.total_ms();
    R->st.ms_total = t_total.total_ms();
    return R.release();
}

}  // namespace fy
