// fy_rm2.hip -- the RM2 relevance-model job on MI355X: statistics, per-cluster M matrix, p(i|u) scoring, top-N.
//
// Math (SURVEY.md section 8a "RM2 in one place"; reference M/rm/AbstractRM2Reducer.java:185-190, 321-371, 384-389):
//     c_vi       = (1-l) r_vi / s_v + l p_i                                  (probItemGivenUser, :384-389)
//     score(u,i) = (n-1) ln M - n ln U_c + sum_{j in rated(u)} ln( sum_{v != u} c_vi c_vj )   for i unrated by u
// The reference evaluates the inner sum with U_c - 1 multiply-adds per (i, j).  Here it is hoisted: for i NOT rated by u
// (x_ui = 0, x = r/s)
//     sum_{v != u} c_vi c_vj = M[j][i] + (l p_i) * e_uj
//     M[j][i] = (1-l)^2 (X^T X)_ij + l (1-l) p_j b_i          per cluster, dense fp32 in HBM, b_i = sum_v x_vi
//     e_uj    = (1-l) (b_j - x_uj) + l (U_c - 1) p_j           per rating of u (= sum_{v != u} c_vj), fp32
// Every term of that form is non-negative, so there is no cancellation even for 2-user clusters; U_c = 1 gives
// exactly 0 -> ln 0 = -inf like the reference (quirk Q7).  Logs are v_log_f32 (base 2, scaled by ln 2 at the end);
// eight of them are added in fp32 and folded into an fp64 running sum, which keeps the relative error of a
// 10^4-term score near 1e-7 (tolerance of north_star: 1e-5).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "fy_cooc.hpp"
#include "fy_prep.hpp"
#include <chrono>
#include "fy_rm2.hpp"
#include "fy_rm2_plan.hpp"
#include "fy_rm1.hpp"
#include "fy_rm2_request.hpp"

namespace fy {

// ================================================================ statistics (jobs RM2-1 / RM2-2)
// One walk over the CSC gives everything that is summed per (cluster, item) column: this rank's PARTIAL rating sum (users
// in slots [lo, hi), the exchange buffer), b = sum_v r_vi / s_v, and the row kernel's work model sum_v n_v.
// Columns are processed in popularity-rank order.  A wave owns a column of up to PAIR_HEAVY raters; the few heavier
// columns (the most popular item of ML-25M shape has ~10^5 raters: one wave would walk it for a millisecond) are
// appended to a list and taken by whole workgroups in k_pair_pass_heavy.  Every column is reduced in a fixed order.
constexpr int PAIR_HEAVY = 2048;
struct PairPass {
    const int32_t* __restrict__ rank_pair;
    const int32_t* __restrict__ pair_start;
    const int32_t* __restrict__ pair_di;
    const int32_t* __restrict__ csc_slot;
    const float* __restrict__ csc_r;
    const double2* __restrict__ ud_slot;   // [slot] = (s_v, n_v): ONE 16-byte gather per entry (the pass runs at the L2's request rate)
    int32_t lo, hi;
    // x = r / s_v per CSC entry (the walk's weights, fy_cooc.hpp) written on the way -- the gather of s_v is this pass's anyway (round 4:
    // a kernel of its own, k_csc_x, with the same 25 M gathers); x / s_v only for the packed walk (null otherwise)
    float* __restrict__ csc_x;
    float* __restrict__ csc_x_over_s;
    double* __restrict__ partial;      // by dense item (several clusters may add to one item)
    double* __restrict__ b_rank;       // by rank position
    long long* __restrict__ walk_rank; // by rank position: sum of the raters' degrees
    int32_t* __restrict__ cnt_rank;    // by rank position: raters
    float* __restrict__ fx_rank;       // by rank position, 3 floats: sum and maximum of r / s_v^2 over the column, maximum rating
                                       // (bounds of the fixed-point scale of the row kernel, fx_exponent)
    // General smoothing (the GEN instantiations; fy_rm2.hpp: Smoothing): ud_slot holds (d_v, n_v), the weights are taken over
    // r' = max(r - delta, 0) (delta = 0: Dirichlet) and d_v, and b_rank receives b~_i = sum_v beta_v x_vi instead of b_i = sum_v x_vi:
    // beta_v x_vi = mu r / d_v^2 (Dirichlet) or delta n_v r' / s_v^2 (absolute discounting), i.e. bt_scale times the sum of the
    // walk weights r' / d_v^2, each multiplied by n_v when bt_by_n -- summed in the same fixed order as b.  The partial rating
    // sums stay those of the raw ratings.
    double delta, bt_scale;
    int32_t bt_by_n;
};
struct PairAcc {   // (no member initialisers: instances live in __shared__ memory too)
    double ps, b, ws;
    long long w;
    float wm, rm;
    double bt;     // general smoothing only
};
__device__ __forceinline__ PairAcc fy_pair_zero() { return PairAcc{0.0, 0.0, 0.0, 0, 0.0f, 0.0f, 0.0}; }
// r' of a rating under absolute discounting, rounded to fp32 like every stored rating (the prepared CSR / CSC hold the same value)
__device__ __forceinline__ float fy_discounted(float r, double delta) { return (float)fmax((double)r - delta, 0.0); }
template <bool GEN>
__device__ __forceinline__ void fy_pair_entry(const PairPass& A, int32_t q, PairAcc& a) {
    const int32_t slot = A.csc_slot[q];
    double r = (double)A.csc_r[q];
    if (slot >= A.lo && slot < A.hi) a.ps += r;
    const double2 ud = A.ud_slot[slot];
    if constexpr (GEN) r = (double)fy_discounted((float)r, A.delta);
    const double inv = 1.0 / ud.x;                    // ONE fp64 division per entry for the column sums (round 4: r / s and r / (s * s) were two;
    const double x = r * inv;                         // the heavy-column kernel ran with 40 spilled VGPRs around them)
    if (A.csc_x || A.csc_x_over_s) {                  // (kernel-uniform) the stored weights keep their own roundings: r / s, then / s
        const double xd = r / ud.x;
        if (A.csc_x) A.csc_x[q] = (float)xd;
        if (A.csc_x_over_s) A.csc_x_over_s[q] = (float)(xd / ud.x);
    }
    a.b += x;
    a.w += (long long)ud.y;
    const double wt = x * inv;
    a.ws += wt;
    if constexpr (GEN) a.bt += A.bt_by_n ? wt * ud.y : wt;
    a.wm = fmaxf(a.wm, (float)wt);
    a.rm = fmaxf(a.rm, (float)r);
}
template <int G = 64, bool GEN = false>
__device__ __forceinline__ void fy_pair_reduce(PairAcc& a) {      // over groups of G consecutive lanes
    for (int o = G / 2; o > 0; o >>= 1) {
        if constexpr (GEN) a.bt += __shfl_down(a.bt, o, 64);
        a.ps += __shfl_down(a.ps, o, 64);
        a.b += __shfl_down(a.b, o, 64);
        a.ws += __shfl_down(a.ws, o, 64);
        a.w += __shfl_down(a.w, o, 64);
        a.wm = fmaxf(a.wm, __shfl_down(a.wm, o, 64));
        a.rm = fmaxf(a.rm, __shfl_down(a.rm, o, 64));
    }
}
template <bool GEN>
__device__ __forceinline__ void fy_pair_store(const PairPass& A, int32_t pos, int32_t pr, int32_t n, const PairAcc& a) {
    if (a.ps != 0.0) atomicAdd(&A.partial[A.pair_di[pr]], a.ps);
    A.b_rank[pos] = GEN ? A.bt_scale * a.bt : a.b;
    A.walk_rank[pos] = a.w;
    A.cnt_rank[pos] = n;
    A.fx_rank[3 * (int64_t)pos + 0] = (float)(a.ws * 1.000001);      // rounded up: these are upper bounds
    A.fx_rank[3 * (int64_t)pos + 1] = a.wm * 1.000001f;
    A.fx_rank[3 * (int64_t)pos + 2] = a.rm;
}
// G lanes per column: 64 for the long columns of a big cluster; 16 where the average column is short (50 clusters of ML-25M shape:
// 2.5 M columns of 10 raters -- a wave per column spent 1.7 ms per job there, four columns per wave 0.5)
// heavy columns are cut into chunks of PAIR_CHUNK entries, one workgroup per chunk (k_pair_chunks), summed per column in chunk order
// (k_pair_finish).  Up to round 4 a workgroup of 1024 walked a whole heavy column: the 10^5-rater columns of ML-25M shape made
// that 0.34 ms of latency-bound tail.
constexpr int PAIR_CHUNK = 4096;
struct PairHeavy {
    int32_t* __restrict__ col;        // [k]: rank position of heavy column k
    int32_t* __restrict__ base;       // [k]: its first chunk
    int32_t* __restrict__ chunk_col;  // [chunk]: k
    int32_t* __restrict__ counters;   // [0] heavy columns, [1] chunks
    PairAcc* __restrict__ acc;        // [chunk]
};
template <int G, bool GEN>
__global__ void k_pair_pass(int32_t nP, PairPass A, PairHeavy H) {
    const int lane = threadIdx.x & (G - 1), gpb = blockDim.x / G;
    const int32_t stride = gridDim.x * gpb;
    // (every group of a wave runs the same number of rounds: the shuffles of the reduction need all lanes)
    for (int32_t pos0 = blockIdx.x * gpb; pos0 < nP; pos0 += stride) {
        const int32_t pos = pos0 + (int32_t)(threadIdx.x / G);
        const bool live = pos < nP;
        const int32_t pr = live ? A.rank_pair[pos] : 0;
        const int32_t q0 = live ? A.pair_start[pr] : 0, q1 = live ? A.pair_start[pr + 1] : 0;
        const bool is_heavy = q1 - q0 > PAIR_HEAVY;
        if (is_heavy && lane == 0) {
            const int32_t nchk = (q1 - q0 + PAIR_CHUNK - 1) / PAIR_CHUNK;
            const int32_t k = atomicAdd(&H.counters[0], 1), c0 = atomicAdd(&H.counters[1], nchk);
            H.col[k] = pos;
            H.base[k] = c0;
            for (int32_t i = 0; i < nchk; i++) H.chunk_col[c0 + i] = k;
        }
        PairAcc a = fy_pair_zero();
        if (!is_heavy)
            for (int32_t q = q0 + lane; q < q1; q += G) fy_pair_entry<GEN>(A, q, a);
        fy_pair_reduce<G, GEN>(a);
        if (live && !is_heavy && lane == 0) fy_pair_store<GEN>(A, pos, pr, q1 - q0, a);
    }
}
template <bool GEN>
__device__ __forceinline__ void fy_pair_add(PairAcc& t, const PairAcc& x) {
    t.ps += x.ps; t.b += x.b; t.ws += x.ws; t.w += x.w;
    t.wm = fmaxf(t.wm, x.wm); t.rm = fmaxf(t.rm, x.rm);
    if constexpr (GEN) t.bt += x.bt;
}
template <bool GEN>
__global__ __launch_bounds__(256) void k_pair_chunks(PairPass A, PairHeavy H) {
    __shared__ PairAcc sh_a[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = H.counters[1];
    for (int c = blockIdx.x; c < n; c += gridDim.x) {
        const int32_t k = H.chunk_col[c];
        const int32_t pr = A.rank_pair[H.col[k]];
        const int32_t q0 = A.pair_start[pr] + (c - H.base[k]) * PAIR_CHUNK, q1 = min(A.pair_start[pr + 1], q0 + PAIR_CHUNK);
        PairAcc a = fy_pair_zero();
#pragma unroll 4
        for (int32_t q = q0 + (int32_t)threadIdx.x; q < q1; q += 256) fy_pair_entry<GEN>(A, q, a);
        fy_pair_reduce<64, GEN>(a);
        if (lane == 0) sh_a[wave] = a;
        __syncthreads();
        if (threadIdx.x == 0) {
            PairAcc t = sh_a[0];
            for (int x = 1; x < 4; x++) fy_pair_add<GEN>(t, sh_a[x]);
            H.acc[c] = t;
        }
        __syncthreads();
    }
}
template <bool GEN>
__global__ void k_pair_finish(PairPass A, PairHeavy H) {
    const int n = H.counters[0];
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const int32_t pos = H.col[k], pr = A.rank_pair[pos];
        const int32_t len = A.pair_start[pr + 1] - A.pair_start[pr], nchk = (len + PAIR_CHUNK - 1) / PAIR_CHUNK;
        PairAcc t = H.acc[H.base[k]];
        for (int32_t i = 1; i < nchk; i++) fy_pair_add<GEN>(t, H.acc[H.base[k] + i]);      // chunk order: the same sum in every run
        fy_pair_store<GEN>(A, pos, pr, len, t);
    }
}
// per-slot copies of the user sums and degrees: one gather per CSC entry instead of two dependent ones
__global__ void k_slot_user_arrays(int32_t nU, const int32_t* __restrict__ slot2du, const double* __restrict__ usum,
                                   const int32_t* __restrict__ udeg, double* __restrict__ usum_slot, int32_t* __restrict__ deg_slot,
                                   double2* __restrict__ ud_slot) {
    for (int32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nU; s += gridDim.x * blockDim.x) {
        const int32_t du = slot2du[s];
        usum_slot[s] = usum[du];
        deg_slot[s] = udeg[du];
        ud_slot[s] = make_double2(usum[du], (double)udeg[du]);
    }
}
// general smoothing: (d_v, n_v) and beta_v of every slot; usum_slot then holds d_v, the divisor of every weight of the job
__global__ void k_slot_user_arrays_gen(int32_t nU, const int32_t* __restrict__ slot2du, const double* __restrict__ usum,
                                       const int32_t* __restrict__ udeg, int method, double param, double* __restrict__ d_slot,
                                       int32_t* __restrict__ deg_slot, double2* __restrict__ ud_slot, double* __restrict__ beta_slot) {
    for (int32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nU; s += gridDim.x * blockDim.x) {
        const int32_t du = slot2du[s];
        const double sv = usum[du], n = (double)udeg[du];
        const double d = method == 1 ? sv + param : sv;
        d_slot[s] = d;
        deg_slot[s] = udeg[du];
        ud_slot[s] = make_double2(d, n);
        beta_slot[s] = method == 1 ? param / d : param * n / sv;
    }
}
// S2 = sum of beta_v^2 over the users of a cluster: one workgroup per cluster, a strided sum per thread, then a tree -- a fixed order
__global__ __launch_bounds__(256) void k_cluster_s2(const int32_t* __restrict__ ucstart, const double* __restrict__ beta_slot, double* __restrict__ s2) {
    __shared__ double sh[256];
    const int c = blockIdx.x;
    double t = 0.0;
    for (int32_t s = ucstart[c] + (int32_t)threadIdx.x; s < ucstart[c + 1]; s += 256) t += beta_slot[s] * beta_slot[s];
    sh[threadIdx.x] = t;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) s2[c] = sh[0];
}
// absolute discounting: the prepared CSR / CSC of the job hold r' = max(r - delta, 0) once the statistics pass has read the raw ratings
__global__ void k_discount_inplace(int64_t n, double delta, float* __restrict__ a, float* __restrict__ b) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        a[q] = fy_discounted(a[q], delta);
        b[q] = fy_discounted(b[q], delta);
    }
}
// ... and whether every r' is exactly representable in fp16 (Prepared::ratings_fp16_exact is then judged on r'): flag[0] = 1 if not
__global__ void k_discount_not_fp16(int64_t n, double delta, const float* __restrict__ r, int32_t* __restrict__ flag) {
    bool bad = false;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const float v = fy_discounted(r[q], delta);
        bad |= __half2float(__float2half(v)) != v;
    }
    if (bad) atomicOr(flag, 1);
}

// per cluster: maxima over its items of (sum of r / s^2, largest r / s^2, largest rating) -> bounds of a Gram entry and of one contribution
__global__ void k_cluster_fx_bounds(const int32_t* __restrict__ pcstart, const float* __restrict__ fx_rank, float* __restrict__ out) {
    // blockIdx.x = cluster, blockIdx.y = share of its items; `out` is zeroed by the caller and the values are >= 0, so the maximum of
    // their bit patterns is their maximum (one cluster of 59 047 items in ONE workgroup was 67 us of every prepare)
    const int c = blockIdx.x;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f;
    for (int32_t pos = pcstart[c] + blockIdx.y * blockDim.x + threadIdx.x; pos < pcstart[c + 1]; pos += gridDim.y * blockDim.x) {
        m0 = fmaxf(m0, fx_rank[3 * (int64_t)pos]);
        m1 = fmaxf(m1, fx_rank[3 * (int64_t)pos + 1]);
        m2 = fmaxf(m2, fx_rank[3 * (int64_t)pos + 2]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        m0 = fmaxf(m0, __shfl_down(m0, o, 64));
        m1 = fmaxf(m1, __shfl_down(m1, o, 64));
        m2 = fmaxf(m2, __shfl_down(m2, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (m0 > 0.f) atomicMax(reinterpret_cast<int*>(out + 3 * c), __float_as_int(m0));
        if (m1 > 0.f) atomicMax(reinterpret_cast<int*>(out + 3 * c + 1), __float_as_int(m1));
        if (m2 > 0.f) atomicMax(reinterpret_cast<int*>(out + 3 * c + 2), __float_as_int(m2));
    }
}

// quirk Q1: the Hadoop counter adds (long) s_u * 100 per user and is divided by 100 afterwards
// (DoubleSumAndCountReducer.java:41, RM2Job.java:95): the total is sum_u floor(s_u).
__global__ void k_partial_total(int32_t lo, int32_t hi, const int32_t* __restrict__ slot2du, const double* __restrict__ usum,
                                unsigned long long* __restrict__ counter) {
    unsigned long long local = 0;
    for (int32_t s = lo + blockIdx.x * blockDim.x + threadIdx.x; s < hi; s += gridDim.x * blockDim.x)
        local += (unsigned long long)((long long)usum[slot2du[s]] * 100LL);
    for (int o = 32; o > 0; o >>= 1) local += __shfl_down(local, o, 64);
    __shared__ unsigned long long sh[16];      // one atomic per workgroup (2 540 waves on one address were most of this kernel's 33 us)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); w++) local += sh[w];
        if (local) atomicAdd(counter, local);
    }
}
__global__ void k_store_total(const unsigned long long* __restrict__ counter, double* __restrict__ dst) {
    *dst = (double)*counter;   // exact below 2^53; the division by OFFSET = 100 happens after the exchange
}

// fixed rank order => bit-reproducible regardless of how the all-gather was scheduled
__global__ void k_sum_gathered(int64_t len, int32_t world, const double* __restrict__ gathered, double* __restrict__ out) {
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < len; d += (int64_t)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int r = 0; r < world; r++) s += gathered[(int64_t)r * len + d];
        out[d] = s;
    }
}

// Sharded prep (whole clusters per rank, only the owned clusters' ratings prepared): a rank's dense item / user numbering is its own,
// so the exchange buffer is laid out by RAW id -- [max_item + 1 item sums][counter][max_user + 1 user sums][failure flag] -- and the
// job's own dense statistics are read back out of the sum over ranks.
__global__ void k_stats_to_raw(int32_t nI, const int32_t* __restrict__ iid, const double* __restrict__ partial, int64_t n_raw_items, int32_t nU,
                               const int32_t* __restrict__ uid, const double* __restrict__ usum, double* __restrict__ raw) {
    const int32_t n = max(nI + 1, nU);
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        if (t < nI) raw[iid[t]] = partial[t];
        if (t == nI) raw[n_raw_items] = partial[nI];
        if (t < nU) raw[n_raw_items + 1 + uid[t]] = usum[t];
    }
}
__global__ void k_stats_from_raw(int32_t nI, const int32_t* __restrict__ iid, const double* __restrict__ raw, int64_t n_raw_items,
                                 double* __restrict__ stats) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t <= nI; t += gridDim.x * blockDim.x) stats[t] = t < nI ? raw[iid[t]] : raw[n_raw_items];
}
__global__ void k_rank_flags(int32_t world, int64_t len, const double* __restrict__ gathered, double* __restrict__ out) {
    if ((int)threadIdx.x < world) out[threadIdx.x] = gathered[(int64_t)threadIdx.x * len + len - 1];
}
__global__ void k_flag_positive(int64_t n, const double* __restrict__ v, uint32_t* __restrict__ flag) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) flag[t] = v[t] > 0.0 ? 1u : 0u;
}
// (id, value * scale) of the positive entries, ascending id
__global__ void k_compact_positive(int64_t n, const double* __restrict__ v, const uint32_t* __restrict__ pos, const double* __restrict__ divide_by,
                                   int32_t* __restrict__ id, double* __restrict__ val) {
    const double d = divide_by ? *divide_by : 1.0;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        if (v[t] > 0.0) {
            id[pos[t] - 1] = (int32_t)t;
            val[pos[t] - 1] = divide_by ? v[t] / d : v[t];
        }
}

// p(i|C) = itemsum / totalSum (DoubleSumAndDividerReducer.java:35-44); stats[nI] holds the counter (x100)
__global__ void k_item_coll(int32_t nI, const double* __restrict__ stats, double* __restrict__ icoll, double* __restrict__ total_out) {
    const double total = stats[nI] / 100.0;
    for (int32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < nI; d += gridDim.x * blockDim.x) icoll[d] = stats[d] / total;
    if (blockIdx.x == 0 && threadIdx.x == 0) *total_out = total;
}

// p(i|C) of every (cluster, item) in rank order, a = l * p, b rounded once to fp32
template <bool GEN>      // GEN (general smoothing): a = p, and b_rank is b~
__global__ void k_pair_p(int32_t nP, const int32_t* __restrict__ rank_pair, const int32_t* __restrict__ pair_di,
                         const double* __restrict__ icoll, double lambda, const double* __restrict__ b_rank,
                         double* __restrict__ p_rank, float* __restrict__ a_rank, float* __restrict__ b_rank32, double2* __restrict__ pb_rank) {
    for (int32_t pos = blockIdx.x * blockDim.x + threadIdx.x; pos < nP; pos += gridDim.x * blockDim.x) {
        const double p = icoll[pair_di[rank_pair[pos]]];
        p_rank[pos] = p;
        pb_rank[pos] = make_double2(p, b_rank[pos]);      // (p, b) side by side: k_csr_values gathers both with one 16-byte load per rating
        if constexpr (GEN) a_rank[pos] = (float)p;
        else a_rank[pos] = (float)(lambda * p);
        b_rank32[pos] = (float)b_rank[pos];
    }
}

// x = r / s_v per CSC entry; for the packed row kernel also x / s_v (the CSR side then carries the raw rating)
__global__ void k_csc_x(int64_t nnz, const int32_t* __restrict__ csc_slot, const float* __restrict__ csc_r,
                        const double* __restrict__ usum_slot, float* __restrict__ csc_x, float* __restrict__ csc_x_over_s) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * blockDim.x) {
        const double s = usum_slot[csc_slot[q]];
        const double x = (double)csc_r[q] / s;
        csc_x[q] = (float)x;
        if (csc_x_over_s) csc_x_over_s[q] = (float)(x / s);
    }
}

// row (popularity rank inside its cluster) of every CSC entry: the symmetric walk cuts a rater's slice behind it
__global__ void k_csc_rank(int64_t nnz, const int32_t* __restrict__ csc_pair, const int32_t* __restrict__ pair_rank, int32_t* __restrict__ out) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * blockDim.x) out[q] = pair_rank[csc_pair[q]];
}

#include "fy_cooc_tables.hpp"   // the walk tables of the row kernel: their kernels and the one host sequence that builds them (part of this translation unit)

// one wave per user row: x = r / s_u and e = (1-l)(b_j - x) + l (U_c - 1) p_j  (all fp64, rounded once)
// GEN (general smoothing): x = r' / d_u, e = e~_uj (fy_e_general), q = p_j; csr_r holds r', pb_rank (p, b~), usum_slot d by slot
template <bool GEN>
__global__ void k_csr_values(int32_t nU, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr_idx,
                             const float* __restrict__ csr_r, const int32_t* __restrict__ slot2du,
                             const int32_t* __restrict__ ucluster, const double* __restrict__ usum,
                             const int32_t* __restrict__ csize, const int32_t* __restrict__ pcstart,
                             const double2* __restrict__ pb_rank, double lambda,
                             const float* __restrict__ gscale /* [cluster]: 2^-c of the packed matrix format, 1 for fp32 rows */,
                             float* __restrict__ csr_x, float* __restrict__ csr_e, float* __restrict__ csr_q,
                             const double* __restrict__ usum_slot, SmoothArgs G) {
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    for (int32_t s = blockIdx.x * wpb + (threadIdx.x >> 6); s < nU; s += gridDim.x * wpb) {
        const int32_t du = slot2du[s];
        const int32_t c = ucluster[du];
        const double sum = GEN ? usum_slot[s] : usum[du];
        const double Uc1 = (double)(csize[c] - 1);
        const double gs = (double)gscale[c];
        const int32_t pb = pcstart[c];
        for (int32_t f = rowptr[s] + lane; f < rowptr[s + 1]; f += 64) {
            const int32_t j = csr_idx[f];
            const double x = (double)csr_r[f] / sum;
            const double2 pbj = pb_rank[pb + j];       // (p(j|C), b_j)
            if constexpr (GEN) {
                const double e = fy_e_general(pbj.y, pbj.x, (double)csr_r[f], sum, (double)G.deg_slot[s], G.beta_slot[s], G.s2_cluster[c], G.bt_scale, G.bt_by_n);
                csr_x[f] = (float)x;
                csr_e[f] = (float)(e * gs);
                csr_q[f] = (float)(pbj.x * gs);
                continue;
            }
            double e = (1.0 - lambda) * (pbj.y - x) + lambda * Uc1 * pbj.x;
            if (!(e > 0.0)) e = 0.0;
            csr_x[f] = (float)x;
            csr_e[f] = (float)(e * gs);
            csr_q[f] = (float)(lambda * (1.0 - lambda) * pbj.x * gs);     // q_j: the rank-one part of a term is q_j b_i
        }
    }
}

// per slot of this rank: pvpi, whether the user gets a list, how many rows it emits
__global__ void k_user_meta(int32_t lo, int32_t hi, const int32_t* __restrict__ slot2du, const int32_t* __restrict__ uid,
                            const int32_t* __restrict__ ucluster, const int32_t* __restrict__ udeg,
                            const int32_t* __restrict__ csize, const int32_t* __restrict__ pcstart, int32_t number_of_items,
                            int32_t top_n, int32_t filter_users, const int32_t* __restrict__ cshift /* [cluster]: c of the packed format */,
                            double* __restrict__ pvpi, int32_t* __restrict__ n_out,
                            unsigned long long* __restrict__ counters /* [0] log terms, [1] users scored */) {
    unsigned long long terms = 0, scored = 0;
    for (int32_t s = lo + blockIdx.x * blockDim.x + threadIdx.x; s < hi; s += gridDim.x * blockDim.x) {
        const int32_t du = slot2du[s];
        const int32_t c = ucluster[du];
        const int32_t n = udeg[du];
        const int32_t Ic = pcstart[c + 1] - pcstart[c];
        const int32_t unrated = Ic - n;
        // AbstractRM2Reducer.java:327-329
        // (+ n c ln 2: the n log terms of a user of a cluster with a scaled matrix are each short by c bits, see FY_P24_SHIFT)
        pvpi[s - lo] = (double)(n - 1) * log((double)number_of_items) - (double)n * log((double)csize[c]) +
                       (double)n * (double)cshift[c] * 0.69314718055994530942;
        // :210-213 (no unrated item -> skipped with a warning), :221-223 (filterUsers)
        const bool skip = unrated <= 0 || uid[du] < filter_users;
        int32_t k = skip ? 0 : min(top_n, unrated);
        if (k < 0) k = 0;
        n_out[s - lo] = k;
        if (!skip) { terms += (unsigned long long)n * (unsigned long long)unrated; scored++; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        terms += __shfl_down(terms, o, 64);
        scored += __shfl_down(scored, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (terms) atomicAdd(&counters[0], terms);
        if (scored) atomicAdd(&counters[1], scored);
    }
}

// ================================================================ G build: co-rating row kernel + RM2 epilogue
// G[j][i] = (1-l)^2 (X^T X)_ji, the pure co-rating Gram (the rank-one part l (1-l) p_j b_i of the reference's inner sum is
// applied by the scoring kernels): symmetric, exactly zero for never co-rated pairs.
// Packed matrix format (clusters with >= pack24_min_items items): 3 bytes per element = 7 exponent + 17 mantissa bits of the fp32
// value, no sign (G >= 0) and no top exponent bit: every stored value is < 2.  The cluster's matrix is stored SCALED by
// 2^-c, c from an upper bound of its largest entry (rm2_score: cluster_scale); the scoring kernels never undo the scale -- q_j
// and e_uj are stored scaled by the same 2^-c, so every term G + q b + a e comes out scaled, its log2 is short by c, and the
// user's pvpi carries + n c ln 2.  Round 2 stored e8m16 (one mantissa bit less): the worst relative error of a score against the
// fp64 definition was 7.3e-6 of north_star's 1e-5; the 17th bit halves the rounding of every matrix element at the same 3 bytes.
constexpr int FY_P24_SHIFT = 6;      // float bits = packed << 6
struct MEpilogue {
    float* __restrict__ M;
    int64_t ldm;
    float w2;     // (1-l)^2
    double fx_inv;   // fixed-point accumulators: (1-l)^2 / fx_scale
    int pack24;   // 3 bytes per element: 8 exponent + 16 mantissa bits of the (non-negative) fp32, rounded to nearest
    float* __restrict__ Bmax;   // optional [row][ldb] in the 24-bit packed format (3 bytes per entry): maximum of the (rounded) row
                                // over every 256-column block
    int64_t ldb;
    int local_rows;   // 1: M / Bmax hold only this launch's rows, k-th row of the launch at index k (cooperative ranks)
    // column-panel mode (fy_rm2_kernels.hpp, "many clusters"): only the first panel_cols columns of a row are stored (row pitch
    // panel_cols), and the block maxima are taken over 64-column sub-blocks of the WHOLE row
    int32_t panel_cols;          // 0 = off
    float* __restrict__ Bmax64;  // [row][ldb64], 3 bytes per entry
    int64_t ldb64;
    // [row][ldb64]: (second largest value of the sub-block, 24 bits) << 8 | column of the largest inside the sub-block; written with
    // every non-zero Bmax64 entry.  k_bound_repair: a user who rated the column of the maximum is bounded by the second value
    uint32_t* __restrict__ Brep;
    // tail-bound launches of panel mode (k_tail_blocks below): the "matrix" is a column range of Bmax64 -- ldm columns are
    // written per row, the rows are `pitch` elements apart (0: the pitch is the row length) and the 24-bit rounding goes up
    int64_t pitch;
    int ceil24;
    // UNROUNDED fp64 copies of the rows the refinement pass reads (k_refine_rows, round 4; the fixed-point sums are exact, so these are
    // the matrix elements to 2^-53): the first head_rows rows of the matrix, whole, at
    // pitch ld_head (symmetric walks: only the columns behind the row are meaningful), and -- symmetric panel mode, whose head rows
    // are not walked over the tail rows' columns -- the first 256 columns of every row from tail_from on.  nullptr = off.
    // The walk from the unpopular side (CoocArgs::half == 2) keeps tail32 the same way for the rows behind the first chunk (tail_from = CH),
    // from their items in front of their own chunk; head32 is then CH columns wide where the head rows all lie in the first chunk.
    double* __restrict__ head32;      // (fp64 since the first measurement: fp32 values left 4e-5 on a forced-small row with |score| = 0.15)
    int64_t ld_head;
    int32_t head_rows;
    double* __restrict__ tail32;
    int32_t tail_from;
    // fp64 accumulators (the unpacked walk, FY_COOC_FX=0): the scale of those copies in fp64 -- w2 is its fp32 rounding, which would leave
    // 6e-8 relative on every copied element; the sums themselves are ds_add_f64 sums, good to a few 2^-53 in whatever order they came
    double w2d;
};

// Cross-lane maxima of the epilogue without an LDS instruction (as ds_bpermute shuffles the six steps of a 64-lane maximum were six
// dependent LDS round trips per loop trip, a sixth of the kernel's LDS instructions): rotations inside the rows of 16 lanes by DPP, then
// v_permlane16_swap across the two rows of a half-wave and v_permlane32_swap across the halves.  With both operands the same register a
// swap leaves "mine" in one result and "the other row's" in the other, whichever way round: their maximum is the maximum of the pair.
// Every lane of the wave must be active at the swaps (the callers' loops are wave-uniform where they take a maximum).
#define FY_ROR16(x, n) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(x), 0x120 + (n), 0xF, 0xF, false))
__device__ __forceinline__ uint32_t fy_max_half_wave(uint32_t m) {      // maximum over the lanes 0-31 / 32-63, in every lane of the half
    m = max(m, FY_ROR16(m, 8));
    m = max(m, FY_ROR16(m, 4));
    m = max(m, FY_ROR16(m, 2));
    m = max(m, FY_ROR16(m, 1));
    const auto r = __builtin_amdgcn_permlane16_swap(m, m, false, false);
    return max((uint32_t)r[0], (uint32_t)r[1]);
}
__device__ __forceinline__ uint32_t fy_max_wave(uint32_t m) {
    m = fy_max_half_wave(m);
    const auto r = __builtin_amdgcn_permlane32_swap(m, m, false, false);
    return max((uint32_t)r[0], (uint32_t)r[1]);
}

// Epilogue of one (row, chunk) item of the RM2 row kernel: G[i][chunk] = w2 * acc -> 24-bit pack (or fp32), the block maxima, and the
// accumulators re-zeroed in the same pass.  All threads of the workgroup; `id` = (row of the launch << 8) | chunk.
// the 24-bit branch of the epilogue; COPY: this item also stores the unrounded fp64 images of its values for the refinement pass
// (MEpilogue::head32 / tail32) -- a separate instantiation, so that the items that do not (all but the first few hundred rows) run
// the code of round 3 (with the stores in the one loop the row kernel took 8.3 instead of 8.1 ms)
// EPI (FY_COOC_EPI): 1 = the plain 24-bit items (no panel, no sub-block maxima, no refinement copy: every item of a one-cluster job but the
// head rows') take eight columns per lane, and the block maxima of both loops are taken without LDS; 0 = the loop of rounds 3-4 alone,
// with its __shfl_xor maximum.  Same bytes either way: every element goes through the same roundings, and a maximum has no order.
// does a plain item (no refinement copy through the four-column loop) take the eight-column loop?
template <class ACC, int EPI>
__device__ __forceinline__ bool cooc_epilogue_takes_eight(const CoocArgs& A, const MEpilogue& E) {
    return EPI && sizeof(ACC) == 8 && A.acc_quarter && !(A.acc_quarter & 1) && !E.Bmax64 && !E.panel_cols && !E.pitch;
}
// The head columns of an item that takes the eight-column loop, unrounded, to tail32 (the refinement pass; the walk from the unpopular side:
// the items in front of the row's own chunk, c0 = the item's first stored column) -- IN FRONT of that loop and with its assignment of columns
// to threads (lane L of wave w: c0 + 512 w + 8 L ... + 7, then every blockDim * 8 columns), so that a thread reads here exactly what it
// reads and zeroes there: no barrier between the two, and the loop of every other item stays as it is.  The same expressions as the
// copying four-column loop's.
template <class ACC>
__device__ __forceinline__ void cooc_rm2_tail_copy(const CoocArgs& A, const MEpilogue& E, const ACC* __restrict__ acc, int row, int c0, int c_end) {
    double* __restrict__ tp = E.tail32 + (int64_t)(row - E.tail_from) * E.head_rows;
    for (int col = c0 + (int)(threadIdx.x >> 6) * 512 + (int)(threadIdx.x & 63) * 8; col < c_end; col += (int)blockDim.x * 8) {
        double t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const ACC a = acc[cooc_acc_index(col - c0 + k, A.acc_quarter)];
            if constexpr (std::is_integral<ACC>::value) t[k] = (double)a * E.fx_inv;
            else t[k] = E.w2d * (double)a;
        }
        double2* __restrict__ o = reinterpret_cast<double2*>(tp + col);
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = make_double2(t[2 * k], t[2 * k + 1]);
    }
}
template <class ACC, bool COPY, int EPI>
__device__ __forceinline__ void cooc_rm2_epilogue_pack(const CoocArgs& A, const MEpilogue& E, ACC* __restrict__ acc, int row, int mrow, int c0, int c1, int cb,
                                                       int first_bmax_block) {
        const int64_t row_cols = E.pitch ? E.pitch : (E.panel_cols ? E.panel_cols : E.ldm);
        const uint32_t radd = E.ceil24 ? (1u << FY_P24_SHIFT) - 1u : 1u << (FY_P24_SHIFT - 1);
        if constexpr (EPI && !COPY && sizeof(ACC) == 8) {
        // Eight columns per lane (planar accumulators; cb, c0 and c1 are multiples of 64): lane L of wave w owns the columns
        // cb + 512 (w + trip * waves) + 8 L ... + 7.  In plane q these are two adjacent words (the columns + q and + 4 + q): one 16-byte
        // read and one 16-byte zeroing write per plane; 24 contiguous bytes of the row per lane.  A half-wave is 256 columns: one block
        // of Bmax when that is requested (cb, c0, c1 are then multiples of 256, pick_chunks), and a half-wave at or behind c1 is masked.
        // The loop is wave-uniform; the reads of the next trip are issued before the arithmetic of this one.
        if (A.acc_quarter && !(A.acc_quarter & 1) && !E.Bmax64 && !E.panel_cols && !E.pitch) {
            // (integral sums as four dwords: low and high halves of the two words, converted from 32 bits each)
            using Pair = typename std::conditional<std::is_integral<ACC>::value, uint4, double2>::type;
            const int qz = A.acc_quarter;
            char* __restrict__ out = reinterpret_cast<char*>(E.M) + (int64_t)mrow * E.ldm * 3;
            const int l8 = (int)(threadIdx.x & 63) * 8, step = (int)blockDim.x * 8;
            int cw = cb + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * 512;         // first column of the wave's trip
            // (a masked lane reads what the last lane in front of c1 reads -- a lane of its own wave, c1 - 8 >= the trip's first column -- and
            // drops it: no branch around the reads, nothing read behind the accumulators)
            auto fetch = [&](int col, Pair* p) __attribute__((always_inline)) {
                const Pair* ap = reinterpret_cast<const Pair*>(acc + ((min(col, c1 - 8) - c0) >> 2));
#pragma unroll
                for (int q = 0; q < 4; q++) p[q] = ap[(q * qz) >> 1];
            };
            auto trip = [&](int col, const Pair* p) __attribute__((always_inline)) {
                const bool on = col < c1;
                if (on) {
                    Pair* ap = reinterpret_cast<Pair*>(acc + ((col - c0) >> 2));
#pragma unroll
                    for (int q = 0; q < 4; q++) ap[(q * qz) >> 1] = Pair{};
                }
                uint32_t v[8];
#pragma unroll
                for (int q = 0; q < 4; q++) {
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        float f;
                        if constexpr (std::is_integral<ACC>::value) {
                            // (double)acc in one rounding: hi * 2^32 is exact, the fma rounds the exact sum once, as the conversion does
                            const double d = __builtin_fma((double)(h ? p[q].w : p[q].y), 4294967296.0, (double)(h ? p[q].z : p[q].x));
                            f = (float)(d * E.fx_inv);
                        } else f = E.w2 * (float)(h ? p[q].y : p[q].x);
                        v[4 * h + q] = (__float_as_uint(f) + radd) >> FY_P24_SHIFT;
                    }
                }
                if (on) {
                    uint32_t* __restrict__ o = reinterpret_cast<uint32_t*>(out + (int64_t)col * 3);
                    o[0] = v[0] | (v[1] << 24);
                    o[1] = (v[1] >> 8) | (v[2] << 16);
                    o[2] = (v[2] >> 16) | (v[3] << 8);
                    o[3] = v[4] | (v[5] << 24);
                    o[4] = (v[5] >> 8) | (v[6] << 16);
                    o[5] = (v[6] >> 16) | (v[7] << 8);
                }
                if (E.Bmax) {
                    uint32_t m = max(max(max(v[0], v[1]), max(v[2], v[3])), max(max(v[4], v[5]), max(v[6], v[7])));
                    m = fy_max_half_wave(on ? m : 0u);
                    if ((threadIdx.x & 31) == 0 && m && (col >> 8) >= first_bmax_block) {
                        uint8_t* bp = reinterpret_cast<uint8_t*>(E.Bmax) + ((int64_t)mrow * E.ldb + (col >> 8)) * 3;
                        bp[0] = (uint8_t)m;
                        bp[1] = (uint8_t)(m >> 8);
                        bp[2] = (uint8_t)(m >> 16);
                    }
                }
            };
            // two register sets take turns (the loop is wave-uniform: cw is a scalar)
            Pair pa[4], pb[4];
            if (cw < c1) fetch(cw + l8, pa);
            while (cw < c1) {
                if (cw + step < c1) fetch(cw + step + l8, pb);
                trip(cw + l8, pa);
                cw += step;
                if (cw >= c1) break;
                if (cw + step < c1) fetch(cw + step + l8, pa);
                trip(cw + l8, pb);
                cw += step;
            }
            return;
        }
        }
        // four columns -> three dwords (c0 and c1 are multiples of 64)
        uint32_t* __restrict__ out3 = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(E.M) + (int64_t)mrow * row_cols * 3);
        for (int c4 = (cb >> 2) + threadIdx.x; 4 * c4 < c1; c4 += blockDim.x) {
            uint32_t v[4];
            // plane q of the accumulators holds the columns = q mod 4 (CoocArgs::acc_quarter): consecutive lanes, consecutive words
            const int qz = A.acc_quarter;
            ACC* ap = acc + (qz ? c4 - (c0 >> 2) : 4 * c4 - c0);
            const int qs = qz ? qz : 1;                       // stride between the four columns of the lane
            double f4[COPY ? 4 : 1];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float f;                                      // columns >= Ic were never touched: 0
                if constexpr (std::is_integral<ACC>::value) { const double d = (double)ap[q * qs] * E.fx_inv; f = (float)d; if constexpr (COPY) f4[q] = d; }
                else { f = E.w2 * (float)ap[q * qs]; if constexpr (COPY) f4[q] = E.w2d * (double)ap[q * qs]; }
                ap[q * qs] = (ACC)0;
                v[q] = (__float_as_uint(f) + radd) >> FY_P24_SHIFT;    // 0 <= f < 2: 7 exponent + 17 mantissa bits, round to nearest (or up)
            }
            // the unrounded values (fp64 images of the fixed-point sums) the refinement pass re-scores ill-conditioned list rows from
            if constexpr (COPY) {
            if (E.head32 && mrow < E.head_rows && 4 * c4 < E.ld_head) {
                double2* hp = reinterpret_cast<double2*>(E.head32 + (int64_t)mrow * E.ld_head + 4 * c4);
                hp[0] = make_double2(f4[0], f4[1]);
                hp[1] = make_double2(f4[2], f4[3]);
            }
            if (E.tail32 && row >= E.tail_from && 4 * c4 < E.head_rows) {
                double2* tp = reinterpret_cast<double2*>(E.tail32 + (int64_t)(row - E.tail_from) * E.head_rows + 4 * c4);
                tp[0] = make_double2(f4[0], f4[1]);
                tp[1] = make_double2(f4[2], f4[3]);
            }
            }
            if (!E.panel_cols || 4 * c4 < E.panel_cols) {
                out3[3 * c4 + 0] = v[0] | (v[1] << 24);
                out3[3 * c4 + 1] = (v[1] >> 8) | (v[2] << 16);
                out3[3 * c4 + 2] = (v[2] >> 16) | (v[3] << 8);
            }
            if (E.Bmax64) {
                // 16 lanes = one 64-column sub-block.  Keys = value << 6 | column inside the sub-block (all different): the two
                // largest keys of the 64, by a four-step butterfly of (first, second) pairs
                const uint32_t cq = (uint32_t)((4 * c4) & 63);
                const uint32_t k0 = (v[0] << 6) | cq, k1 = (v[1] << 6) | (cq + 1), k2 = (v[2] << 6) | (cq + 2), k3 = (v[3] << 6) | (cq + 3);
                const uint32_t a1 = max(k0, k1), a2 = min(k0, k1), b1 = max(k2, k3), b2 = min(k2, k3);
                uint32_t t1 = max(a1, b1), t2 = max(min(a1, b1), max(a2, b2));
                // rotations inside the row of 16 lanes (DPP row_ror: no LDS instruction -- as ds_bpermute shuffles these were a third
                // of the kernel's LDS instructions in a 50-cluster job): after ror 8, 4, 2, 1 every lane has seen all 16, each once
#define FY_TOP2_STEP(n)                                         \
    {                                                           \
        const uint32_t p1 = FY_ROR16(t1, n), p2 = FY_ROR16(t2, n); \
        t2 = max(min(t1, p1), max(t2, p2));                     \
        t1 = max(t1, p1);                                       \
    }
                FY_TOP2_STEP(8) FY_TOP2_STEP(4) FY_TOP2_STEP(2) FY_TOP2_STEP(1)
#undef FY_TOP2_STEP
                const uint32_t m = t1 >> 6;
                if ((threadIdx.x & 15) == 0 && m) {
                    uint8_t* bp = reinterpret_cast<uint8_t*>(E.Bmax64) + ((int64_t)mrow * E.ldb64 + (c4 >> 4)) * 3;
                    bp[0] = (uint8_t)m;
                    bp[1] = (uint8_t)(m >> 8);
                    bp[2] = (uint8_t)(m >> 16);
                    if (E.Brep) E.Brep[(int64_t)mrow * E.ldb64 + (c4 >> 4)] = ((t2 >> 6) << 8) | (t1 & 63u);
                }
            }
            if (E.Bmax) {
                // maximum of the values exactly as the scoring kernel will unpack them; one wave = one 256-column
                // block (c0 and c1 are multiples of 256 when the bound matrix is requested, see pick_chunks)
                uint32_t m = max(max(v[0], v[1]), max(v[2], v[3]));     // non-negative floats order like their bit patterns
                if constexpr (EPI) m = fy_max_wave(m);      // (c1 - cb is a multiple of 256 here: whole waves)
                else {
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
                }
                if ((threadIdx.x & 63) == 0 && m && (c4 >> 6) >= first_bmax_block) {
                    // the maximum of 24-bit values is itself one: Bmax is stored in the same packed format (3 bytes per
                    // block, byte stores: the four blocks of a packed group belong to different waves or chunks), so
                    // the bound pass streams 768 instead of 1024 bytes per rated item.  (Zero maxima are not stored:
                    // the matrix was cleared before the launch.)
                    uint8_t* bp = reinterpret_cast<uint8_t*>(E.Bmax) + ((int64_t)mrow * E.ldb + (c4 >> 6)) * 3;
                    bp[0] = (uint8_t)m;
                    bp[1] = (uint8_t)(m >> 8);
                    bp[2] = (uint8_t)(m >> 16);
                }
            }
        }
}

template <class ACC, int EPI>
__device__ __forceinline__ void cooc_rm2_epilogue(const CoocArgs& A, const MEpilogue& E, ACC* __restrict__ acc, int id) {
    const int lrow = id >> 8;
    const int row = A.row0 + lrow * (A.row_stride ? A.row_stride : 1);
    const int mrow = E.local_rows ? lrow : row;
    const int ch = id & 255;
    const int c0 = ch * A.CH;
    // the last chunk also writes the padding columns [Ic, ldm) so the scoring kernel may load whole 256-wide chunks
    const int c1 = (ch == A.nch - 1) ? (int)E.ldm : min(c0 + A.CH, (int)E.ldm);
    // symmetric walk: in the row's own chunk nothing in front of its 256-column diagonal block was accumulated (and the
    // mirror pass writes that part of the row); the block maxima of the diagonal block are the mirror pass's too
    // (the walk from the unpopular side, half == 2: an item in front of the row's own chunk is a whole chunk, block maxima and all)
    const bool front = A.half == 2 && c0 + A.CH <= row;
    const int cb = (cooc_row_is_cut(A, row) && c0 <= row && !front) ? (row & ~255) : c0;
    const int first_bmax_block = (A.half && !front) ? (row >> 8) + 1 : 0;
    if (E.pack24) {
        // (block-uniform) does this item hold values the refinement pass wants?  Under half == 2 the rows behind the first chunk keep
        // their head columns (tail32), and only in their items in front of their own chunk: ~ (Ic - CH) items of a job, which stay in
        // the eight-column loop where that loop is taken at all (cooc_rm2_tail_copy in front of it) and take the copying loop otherwise
        const bool tail_item = E.tail32 && row >= E.tail_from && c0 < E.head_rows && (A.half != 2 || front);
        const bool tail8 = tail_item && A.half == 2 && cooc_epilogue_takes_eight<ACC, EPI>(A, E);
        const bool copy = E.head32 && (mrow < E.head_rows || (tail_item && !tail8));
        if (copy) cooc_rm2_epilogue_pack<ACC, true, EPI>(A, E, acc, row, mrow, c0, c1, cb, first_bmax_block);
        else {
            if (tail8) cooc_rm2_tail_copy<ACC>(A, E, acc, row, c0, min(c1, (int)E.head_rows));
            cooc_rm2_epilogue_pack<ACC, false, EPI>(A, E, acc, row, mrow, c0, c1, cb, first_bmax_block);
        }
    } else {
        float* __restrict__ out = E.M + (int64_t)mrow * E.ldm;
        for (int col = cb + threadIdx.x; col < c1; col += blockDim.x) {
            const int at = cooc_acc_index(col - c0, A.acc_quarter);
            if constexpr (std::is_integral<ACC>::value) out[col] = (float)((double)acc[at] * E.fx_inv);
            else out[col] = E.w2 * (float)acc[at];
            acc[at] = (ACC)0;
        }
    }
}

// Persistent workgroups pull (row, chunk) items from a global counter (rows are in popularity order: heavy items first);
// the epilogue re-zeroes the accumulators it reads, so an item costs one accumulate phase, one barrier, one epilogue and
// one barrier -- no dispatch, no separate clearing pass.
//
// Round 2: (1) accumulators in fp32 (ds_add_f32, ACC = float): half the LDS per column, so TWO workgroups share a CU and
// one streams rater slices while the other sits in its barrier / epilogue (one 16-wave workgroup per CU spent half of
// every item's 25 us waiting: three dependent round trips in front of the first slice load, then the epilogue).  Today
// (launch_cooc_rm2) ACC is 64-bit fixed point in the packed walk, 32-bit where the sums of the item-similarity Gram fit,
// double otherwise, float only with FY_COOC_F32=1.  (2) The item counter is read TWO items ahead by thread 0, which
// also fetches the segment range of the next item while the current one is accumulated; after the barrier every wave issues
// the load of its first 64 segment descriptors of the NEXT item, and only then runs the epilogue: of the three round
// trips in front of an item's first slice load none is exposed any more.  (3) The epilogue no longer reads b and p.
// ROLE only names the instantiation (kernel traces): 0 = matrix rows, 1 = the tail rows' block bounds of panel mode (k_tail_blocks)
template <bool PK, class ACC, int EPI>
__device__ __forceinline__ void cooc_rm2_body(const CoocArgs& A, const MEpilogue& E, int n_items, int* __restrict__ next_item) {
    ACC* __restrict__ acc = reinterpret_cast<ACC*>(fy_cooc_acc);
    __shared__ int sh_item, sh_s0, sh_s1, sh_id;
    const int CHp = cooc_lds_columns(A.CH);   // allocated (and zeroed) columns: the epilogue reads whole 256-column blocks
    for (int t = threadIdx.x; t < CHp; t += blockDim.x) acc[t] = (ACC)0;
    // items are handed out by a global counter: the chunks of a row differ a lot in weight (chunk 0 holds the popular
    // columns), a static stride would leave three quarters of the workgroups idle behind the chunk-0 owners
    // The counter hands out ITEM_GRAB consecutive items per atomic: one address takes ~82 M device-scope atomics per second on
    // this part (every launch of this kernel over short items ran at exactly that item rate, whatever the chunk width or the
    // walk: 99 k items in 1.20 ms, 46 k in 0.57 ms, 364 k in 4.4 ms), and in a cluster of 3 000 users an item is ~60 segments.
    // The base of the batch after the current one is fetched when a batch is started: its latency never shows.
    // Rows with thousands of segments (one cluster of 162 000 users) keep one item per atomic: eight consecutive items are the
    // chunks of ONE row there, and a batch of them unbalances the tail (7.9 -> 12.7 ms).
    const int ITEM_GRAB = A.item_grab > 0 ? A.item_grab : 1;
    int next = 0, next2 = 0;      // thread 0 only: the next item and the one after it
    int g_cur = 0, g_end = 0, g_next = 0;
    auto grab = [&]() __attribute__((always_inline)) {
        if (g_cur == g_end) {
            g_cur = g_next;
            g_end = g_cur + ITEM_GRAB;
            g_next = atomicAdd(next_item, ITEM_GRAB);
        }
        return g_cur++;
    };
    if (threadIdx.x == 0) {
        g_cur = atomicAdd(next_item, ITEM_GRAB);
        g_end = g_cur + ITEM_GRAB;
        g_next = atomicAdd(next_item, ITEM_GRAB);
        const int first = grab();
        next = grab();
        const int2 se = first < n_items ? A.item_seg[first] : make_int2(0, 0);
        sh_item = first;
        sh_s0 = se.x;
        sh_s1 = se.y;
        sh_id = first < n_items ? A.item_id[first] : 0;
    }
    __syncthreads();
    int item = sh_item, s0 = sh_s0, s1 = sh_s1, id = sh_id;
    // Every wave must have read the first item before thread 0 publishes the second one (it does so as soon as ITS share of
    // the first item is accumulated).  Inside the loop the barrier behind the epilogue separates the two; here nothing did:
    // with other kernels competing for the CU a delayed wave read the second item as its first -- thousands of wrong matrix
    // rows per job, only with several job lanes in flight (tools/debug_margin.py found it).
    __syncthreads();
    SegBatch batch = cooc_first_batch(A, s0, s1);
    while (item < n_items) {     // block-uniform
        int2 se_next = make_int2(0, 0);
        int id_next = 0;
        if (threadIdx.x == 0) {
            next2 = grab();
            if (next < n_items) { se_next = A.item_seg[next]; id_next = A.item_id[next]; }   // address known since the previous item
        }
        const int c0 = (id & 255) * A.CH;
        // symmetric walk: in the row's OWN chunk the slices start at a 64-aligned position in front of the row's column (segment
        // table: k_seg_counts' cut start); the entries at or before it are masked here -- row i accumulates only the columns j > i
        const int row_of_item = A.row0 + (id >> 8) * (A.row_stride ? A.row_stride : 1);
        const int rmask = (cooc_row_is_cut(A, row_of_item) && row_of_item >= c0 && row_of_item < c0 + A.CH) ? row_of_item - c0 : -1;
        if constexpr (PK) cooc_accumulate_pk<ACC>(A, acc, s0, s1, batch, rmask);
        else cooc_accumulate_segments<false, ACC>(A, acc, s0, s1, c0, batch, rmask);
        // (every thread read sh_* of THIS item before the barrier that ended the previous epilogue)
        if (threadIdx.x == 0) { sh_item = next; sh_s0 = se_next.x; sh_s1 = se_next.y; sh_id = id_next; }
        __syncthreads();     // all atomics of this item are done; the next item is published
        const int nitem = sh_item;
        s0 = sh_s0;
        s1 = sh_s1;
        const int nid = sh_id;
        batch = cooc_first_batch(A, s0, s1);     // in flight during the epilogue
        cooc_rm2_epilogue<ACC, EPI>(A, E, acc, id);
        item = nitem;
        id = nid;
        if (threadIdx.x == 0) next = next2;
        __syncthreads();   // the accumulators are clean again before the next item's atomics
    }
}
// EPI: the epilogue's loops (cooc_rm2_epilogue_pack; FY_COOC_EPI)
template <bool PK, class ACC, int ROLE = 0, int EPI = 1>
__global__ void k_cooc_rm2(CoocArgs A, MEpilogue E, int n_items, int* __restrict__ next_item) {
    cooc_rm2_body<PK, ACC, EPI>(A, E, n_items, next_item);
}
// The matrix builds of SEVERAL clusters in one launch (panel mode, many clusters): blockIdx.y = cluster; its arguments and its item
// counter come from device memory.  The workgroups of cluster c + 1 start on the CUs that cluster c's workgroups leave: no launch
// gap and no idle tail between two clusters' row kernels (50 clusters at ML-25M shape: 100 launches back to back were 41 ms).
struct CoocLaunch {
    CoocArgs A;
    MEpilogue E;
    int32_t n_items, pad;
};
template <bool PK, class ACC, int ROLE = 0, int EPI = 1>
__global__ void k_cooc_rm2_multi(const CoocLaunch* __restrict__ D, int* __restrict__ counters) {
    const CoocLaunch& d = D[blockIdx.y];
    const CoocArgs A = d.A;
    const MEpilogue E = d.E;
    cooc_rm2_body<PK, ACC, EPI>(A, E, d.n_items, counters + blockIdx.y);
}
// the item lists of all those launches (CoocArgs::item_seg / item_id name the lists to fill)
__global__ void k_item_list_multi(const CoocLaunch* __restrict__ D) {
    const CoocArgs A = D[blockIdx.y].A;
    item_list_body(A, const_cast<int2*>(A.item_seg), const_cast<int32_t*>(A.item_id));
}

// ================================================================ mirror pass of the symmetric (half) walk
// After k_cooc_rm2 with CoocArgs::half, row i of the packed matrix holds the columns j >= 256 * (i / 256) (exact for j > i,
// zero elsewhere in the diagonal block) and Bmax holds the blocks behind the diagonal block.  G is symmetric, so the rest is
// a transposition: 24-bit elements, 256 x 128 source tiles through LDS (k_mirror_tiles: reads 256 row segments of 384 B,
// writes 128 row segments of 768 B -- one whole 256-column block of the destination rows, whose maximum is the missing
// Bmax entry), and the 256 x 256 diagonal blocks thread by thread (k_mirror_diag: 1 / 231 of the matrix).
// After the walk from the unpopular side (CoocArgs::half == 2, `bpc` = 256-column blocks per chunk) the stored off-diagonal tiles are
// those of cooc_tile_stored(B, T, bpc): behind the diagonal block inside the row's own chunk, and every tile of the chunks in front of
// it -- Bmax holds exactly those.  Every kernel below asks that one predicate which tiles are sources; the row blocks of the last
// chunk, the last block too, have sources, and the column blocks of the first chunk (the seed columns) need no tile for the rows of the
// other chunks.  The diagonal blocks are the same either way.
__device__ __forceinline__ void fy_unpack24_raw(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t* v) {
    v[0] = d0 & 0xFFFFFFu;
    v[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8);
    v[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16);
    v[3] = d2 >> 8;
}
__device__ __forceinline__ uint32_t fy_load24(const uint32_t* __restrict__ row3, int e) {   // element e of a packed row
    const int g = e >> 2;
    uint32_t v[4];
    fy_unpack24_raw(row3[3 * g], row3[3 * g + 1], row3[3 * g + 2], v);
    return v[e & 3];
}
constexpr int MIRROR_PITCH = 772;    // bytes per LDS row: 768 + 4 (an odd number of dwords spreads the rows over the banks)

extern __shared__ __attribute__((aligned(16))) unsigned char fy_mirror_lds[];   // [128][MIRROR_PITCH]: the destination rows, packed
// `need` / `write_below` (round 4, the LAZY mirror of the pruned one-cluster job): the transposed tile is stored only for the column blocks
// somebody reads -- B < write_below (the seed columns) or need[B] != 0 (blocks with survivors, flagged on the device by
// k_flag_surviving_blocks) -- while the block maxima (Bmax_ != nullptr) are taken from every tile.  The full mirror is write_below =
// INT_MAX.  Measured: the survivors of the headline job (22 600 (user, block) pairs) lie in 8 of its 231 column blocks.
__device__ __forceinline__ void mirror_tiles_body(float* __restrict__ M_, int64_t ldm, int32_t Ic, float* __restrict__ Bmax_, int64_t ldb,
                                                  const int32_t* __restrict__ need = nullptr, int32_t write_below = 0x7FFFFFFF,
                                                  int32_t bpc = 0 /* blocks per chunk of the walk from the unpopular side, 0 = the plain half walk */) {
    __shared__ uint32_t rowmax[128];
    const int tj = blockIdx.x, B = blockIdx.y;
    if ((tj >> 1) == B || !cooc_tile_stored(B, tj >> 1, bpc)) return;      // only tiles the walk stored are sources (plain: strictly behind the diagonal block)
    const int dst_row0 = 128 * tj;
    if (dst_row0 >= Ic) return;                           // destination rows are real rows (the padding columns have none)
    const bool write = B < write_below || (need && need[B] != 0);      // block-uniform
    if (!write && !Bmax_) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int64_t pitch = ldm * 3;
    unsigned char* __restrict__ Mb = reinterpret_cast<unsigned char*>(M_);
    if (threadIdx.x < 128) rowmax[threadIdx.x] = 0;
    __syncthreads();
    // ---- load: a wave takes two source rows per step (32 lanes x 12 bytes = 128 elements each)
    const int m = lane & 31, h = lane >> 5;
    uint32_t mx[4] = {0, 0, 0, 0};
    for (int r = 2 * wave + h; r < 256; r += 2 * nwaves) {
        const int src_row = 256 * B + r;
        uint32_t v[4] = {0, 0, 0, 0};
        if (src_row < Ic) {
            const uint32_t* __restrict__ p = reinterpret_cast<const uint32_t*>(Mb + (int64_t)src_row * pitch + (int64_t)dst_row0 * 3) + 3 * m;
            fy_unpack24_raw(p[0], p[1], p[2], v);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (write) {
                unsigned char* d = fy_mirror_lds + (4 * m + q) * MIRROR_PITCH + 3 * r;    // destination row 4m + q, element r
                d[0] = (unsigned char)v[q];
                d[1] = (unsigned char)(v[q] >> 8);
                d[2] = (unsigned char)(v[q] >> 16);
            }
            mx[q] = max(mx[q], v[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (mx[q]) atomicMax(&rowmax[4 * m + q], mx[q]);
    __syncthreads();
    // ---- store: one destination row (768 bytes = one 256-column block) per wave step
    for (int c = wave; write && c < 128; c += nwaves) {
        const int dst_row = dst_row0 + c;
        if (dst_row >= Ic) break;
        const uint32_t* __restrict__ sp = reinterpret_cast<const uint32_t*>(fy_mirror_lds + c * MIRROR_PITCH) + 3 * lane;
        uint32_t* __restrict__ dp = reinterpret_cast<uint32_t*>(Mb + (int64_t)dst_row * pitch + (int64_t)256 * B * 3) + 3 * lane;
        dp[0] = sp[0];
        dp[1] = sp[1];
        dp[2] = sp[2];
    }
    if (Bmax_ && threadIdx.x < 128 && dst_row0 + (int)threadIdx.x < Ic) {
        const uint32_t pv = rowmax[threadIdx.x];
        uint8_t* bp = reinterpret_cast<uint8_t*>(Bmax_) + ((int64_t)(dst_row0 + threadIdx.x) * ldb + B) * 3;
        bp[0] = (uint8_t)pv;
        bp[1] = (uint8_t)(pv >> 8);
        bp[2] = (uint8_t)(pv >> 16);
    }
}

__global__ __launch_bounds__(1024) void k_mirror_tiles(float* __restrict__ M_, int64_t ldm, int32_t Ic, float* __restrict__ Bmax_, int64_t ldb,
                                                       const int32_t* __restrict__ need, int32_t write_below, int32_t bpc) {
    mirror_tiles_body(M_, ldm, Ic, Bmax_, ldb, need, write_below, bpc);
}
// Block maxima alone (lazy mirror, first pass, the column blocks nobody reads below the diagonal): Bmax[j][B] = max over the rows i of block B
// of G[i][j] for the 256 columns j of a tile strictly behind block B.  A wave reads WHOLE 768-byte row segments (one 12-byte load per
// lane, 16 rows in flight per workgroup step) -- the transposing tile kernel reads 384-byte half segments and stages them through LDS,
// which this pass has no use for; the 16 waves' maxima meet in LDS and each thread stores one 3-byte entry.
__global__ __launch_bounds__(1024) void k_colmax_upper(const float* __restrict__ M_, int64_t ldm, int32_t Ic, float* __restrict__ Bmax_, int64_t ldb, int32_t first_block,
                                                       int32_t bpc) {
    __shared__ uint32_t colmax[256];
    const int tj = blockIdx.x, B = first_block + blockIdx.y;      // tile = columns [256 tj, 256 tj + 256) x rows of block B
    if (tj == B || !cooc_tile_stored(B, tj, bpc) || 256 * B >= Ic) return;      // a stored tile (plain: strictly behind the diagonal block)
    const int col0 = 256 * tj;
    if (col0 >= Ic) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t pitch = ldm * 3;
    const unsigned char* __restrict__ Mb = reinterpret_cast<const unsigned char*>(M_);
    if (threadIdx.x < 256) colmax[threadIdx.x] = 0;
    __syncthreads();
    uint32_t mx[4] = {0, 0, 0, 0};
    const int r_end = min(256, Ic - 256 * B);
    uint32_t d[4][3];
#pragma unroll
    for (int step = 0; step < 4; step++) {                         // 16 waves x 16 rows: four loads in flight per lane
#pragma unroll
        for (int x = 0; x < 4; x++) {
            const int r = wave * 16 + step * 4 + x;
            const uint32_t* __restrict__ p = reinterpret_cast<const uint32_t*>(Mb + (int64_t)(256 * B + min(r, r_end - 1)) * pitch + (int64_t)col0 * 3) + 3 * lane;
            d[x][0] = p[0]; d[x][1] = p[1]; d[x][2] = p[2];
        }
#pragma unroll
        for (int x = 0; x < 4; x++) {
            uint32_t v[4];
            fy_unpack24_raw(d[x][0], d[x][1], d[x][2], v);
#pragma unroll
            for (int q = 0; q < 4; q++) mx[q] = max(mx[q], v[q]);      // (a clamped row repeats the block's last row: the maximum is unchanged)
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (mx[q]) atomicMax(&colmax[4 * lane + q], mx[q]);
    __syncthreads();
    if (threadIdx.x < 256 && col0 + (int)threadIdx.x < Ic) {
        const uint32_t pv = colmax[threadIdx.x];
        uint8_t* bp = reinterpret_cast<uint8_t*>(Bmax_) + ((int64_t)(col0 + threadIdx.x) * ldb + B) * 3;
        bp[0] = (uint8_t)pv;
        bp[1] = (uint8_t)(pv >> 8);
        bp[2] = (uint8_t)(pv >> 16);
    }
}
// need[b] = 1 for every block b some user of the batch keeps (the survivor lists of k_bound_select)
__global__ void k_flag_surviving_blocks(int32_t n_users, const int32_t* __restrict__ n_quads, const uint16_t* __restrict__ surv, int64_t ldb, int32_t* __restrict__ need) {
    for (int32_t u = blockIdx.x; u < n_users; u += gridDim.x)
        for (int k = threadIdx.x; k < n_quads[u]; k += blockDim.x) {
            const int b = surv[(int64_t)u * ldb + k];
            if (need[b] == 0) need[b] = 1;      // (benign race: every writer stores 1)
        }
}
// diagonal blocks: thread c owns row 256 B + c; element (c, r) for r < c is element (r, c) of a row above (a 3-byte gather),
// the rest of the row's segment is its own; the maximum over the completed segment is Bmax[row][B]
__device__ __forceinline__ void mirror_diag_body(float* __restrict__ M_, int64_t ldm, int32_t Ic, float* __restrict__ Bmax_, int64_t ldb) {
    const int B = blockIdx.x, c = threadIdx.x;
    const int row = 256 * B + c;
    if (row >= Ic) return;
    const int64_t pitch = ldm * 3;
    unsigned char* __restrict__ Mb = reinterpret_cast<unsigned char*>(M_);
    uint32_t* __restrict__ own = reinterpret_cast<uint32_t*>(Mb + (int64_t)row * pitch + (int64_t)256 * B * 3);
    uint32_t best = 0;
    for (int g = 0; g < 64; g++) {
        uint32_t v[4];
        if (4 * g >= c) {                                  // untouched part of the own row (columns >= c)
            fy_unpack24_raw(own[3 * g], own[3 * g + 1], own[3 * g + 2], v);
        } else {
            if (4 * g + 3 >= c) fy_unpack24_raw(own[3 * g], own[3 * g + 1], own[3 * g + 2], v);   // the group that straddles the diagonal
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r = 4 * g + q;
                if (r < c) v[q] = fy_load24(reinterpret_cast<const uint32_t*>(Mb + (int64_t)(256 * B + r) * pitch + (int64_t)256 * B * 3), c);
            }
            own[3 * g + 0] = v[0] | (v[1] << 24);
            own[3 * g + 1] = (v[1] >> 8) | (v[2] << 16);
            own[3 * g + 2] = (v[2] >> 16) | (v[3] << 8);
        }
        best = max(max(best, max(v[0], v[1])), max(v[2], v[3]));
    }
    if (Bmax_) {
        uint8_t* bp = reinterpret_cast<uint8_t*>(Bmax_) + ((int64_t)row * ldb + B) * 3;
        bp[0] = (uint8_t)best;
        bp[1] = (uint8_t)(best >> 8);
        bp[2] = (uint8_t)(best >> 16);
    }
}

__global__ __launch_bounds__(256) void k_mirror_diag(float* __restrict__ M_, int64_t ldm, int32_t Ic, float* __restrict__ Bmax_, int64_t ldb) {
    mirror_diag_body(M_, ldm, Ic, Bmax_, ldb);
}
// the panels of all clusters of a symmetric panel-mode job: blockIdx.z (tiles, column maxima) / blockIdx.y (diagonal blocks) = cluster
struct PanelDesc {
    float* Gp;
    float* Bmax64;
    uint32_t* Brep;
    int64_t panel_cols, ldb64;
    int32_t Ic, p_eff, nsub, pad;
};
__global__ __launch_bounds__(1024) void k_mirror_tiles_multi(const PanelDesc* __restrict__ D) {
    const PanelDesc d = D[blockIdx.z];
    if ((int)blockIdx.x >= (int)(d.panel_cols / 128) || (int)blockIdx.y >= (int)(d.panel_cols / 256) - 1) return;
    mirror_tiles_body(d.Gp, d.panel_cols, d.p_eff, nullptr, 0);
}
__global__ __launch_bounds__(256) void k_mirror_diag_multi(const PanelDesc* __restrict__ D) {
    const PanelDesc d = D[blockIdx.y];
    if ((int)blockIdx.x >= (int)(d.panel_cols / 256)) return;
    mirror_diag_body(d.Gp, d.panel_cols, d.p_eff, nullptr, 0);
}
// Symmetric panel mode: the sub-block maxima of the HEAD rows (i < p_eff) from the stored panel, by symmetry:
//     Bmax64[i][sb] = max_{j in sub-block sb} G[i][j] = max_j Gp[j][i],      Brep[i][sb] = (second largest << 8) | (j of the largest - 64 sb)
// for every sub-block sb of the row -- the panel Gp holds column i of EVERY row j (head rows after the mirror pass, tail rows from
// their walk over the head chunks).  Work-group = 256 columns x 16 sub-blocks (1024 rows of the panel): wave w takes sub-blocks
// 4 w .. 4 w + 3, a lane four columns (12-byte loads, a wave reads 768 contiguous bytes of a row); the results go through LDS so
// that a thread writes the 16 entries of ONE row of Bmax64 / Brep (48 / 64 contiguous bytes).  Every entry of the head rows is
// written, zeros too: what the row kernel's epilogue left there (sub-blocks of the partly walked own chunk) is overwritten.
__global__ __launch_bounds__(256) void k_panel_colmax(const PanelDesc* __restrict__ D) {
    const PanelDesc dsc = D[blockIdx.z];
    const float* __restrict__ Gp_ = dsc.Gp;
    float* __restrict__ Bmax64_ = dsc.Bmax64;
    uint32_t* __restrict__ Brep = dsc.Brep;
    const int64_t panel_cols = dsc.panel_cols, ldb64 = dsc.ldb64;
    const int32_t Ic = dsc.Ic, p_eff = dsc.p_eff, nsub = dsc.nsub;
    if ((int)blockIdx.x * 256 >= p_eff || (int)blockIdx.y * 16 >= nsub) return;
    __shared__ uint32_t sh_m[16][257], sh_r[16][257];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col0 = blockIdx.x * 256, sbg = blockIdx.y * 16;
    const int c = col0 + 4 * lane;
    const unsigned char* __restrict__ base = reinterpret_cast<const unsigned char*>(Gp_) + (int64_t)c * 3;
    const int64_t pitch = panel_cols * 3;
    for (int s = 0; s < 4; s++) {
        const int sb = sbg + 4 * wave + s;
        uint32_t t1[4] = {0, 0, 0, 0}, t2[4] = {0, 0, 0, 0};
        if (sb < nsub) {
            const int j0 = 64 * sb, nr = min(64, Ic - j0);
            for (int r = 0; r < nr; r += 8) {
                uint32_t d[8][3];
#pragma unroll
                for (int x = 0; x < 8; x++) {
                    const uint32_t* __restrict__ p = reinterpret_cast<const uint32_t*>(base + (int64_t)(j0 + min(r + x, nr - 1)) * pitch);
                    d[x][0] = p[0]; d[x][1] = p[1]; d[x][2] = p[2];
                }
#pragma unroll
                for (int x = 0; x < 8; x++) {
                    if (r + x < nr) {
                        uint32_t v[4];
                        fy_unpack24_raw(d[x][0], d[x][1], d[x][2], v);
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const uint32_t key = (v[q] << 6) | (uint32_t)(r + x);
                            t2[q] = max(min(t1[q], key), t2[q]);
                            t1[q] = max(t1[q], key);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            sh_m[4 * wave + s][4 * lane + q] = t1[q] >> 6;
            sh_r[4 * wave + s][4 * lane + q] = (t1[q] >> 6) ? (((t2[q] >> 6) << 8) | (t1[q] & 63u)) : 0u;
        }
    }
    __syncthreads();
    const int i = col0 + threadIdx.x;
    if (i < p_eff) {
        uint32_t m[16];
#pragma unroll
        for (int k = 0; k < 16; k++) m[k] = sh_m[k][threadIdx.x];
        // 16 entries of 3 bytes = 12 dwords at a 16-byte aligned address (ldb64 and sbg are multiples of 16)
        uint32_t* __restrict__ bp = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(Bmax64_) + ((int64_t)i * ldb64 + sbg) * 3);
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const uint32_t* v = m + 4 * g;
            bp[3 * g + 0] = v[0] | (v[1] << 24);
            bp[3 * g + 1] = (v[1] >> 8) | (v[2] << 16);
            bp[3 * g + 2] = (v[2] >> 16) | (v[3] << 8);
        }
        uint32_t* __restrict__ rp = Brep + (int64_t)i * ldb64 + sbg;
#pragma unroll
        for (int k = 0; k < 16; k++) rp[k] = sh_r[k][threadIdx.x];
    }
}

// full mirror: write_below = INT_MAX.  Lazy mirror, first pass (block maxima from every tile, lower triangle only for the column blocks
// in front of write_below + the diagonal blocks): need = nullptr, write_below = seed blocks.  Second pass (after the survivors are
// known): Bmax = nullptr, need = the flags, write_below = 0, diag = false -- a tile of an unflagged block leaves at once.
// bpc: blocks per chunk of the walk from the unpopular side (0 = the plain half walk): the rows of the LAST block are sources too
static void launch_mirror(Context* ctx, float* M, int64_t ldm, int32_t Ic, float* Bmax, int64_t ldb, hipStream_t st, int bpc, const int32_t* need = nullptr,
                          int32_t write_below = 0x7FFFFFFF, bool diag = true) {
    const int nblk = (int)(ldm / 256), ntile = (int)(ldm / 128);
    const int nsrc = bpc > 0 ? nblk : nblk - 1;      // row blocks with stored tiles
    if (nblk > 1) {
        FY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_mirror_tiles), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * MIRROR_PITCH));
        // first pass of the lazy mirror: the transposing kernel only over the column blocks it writes (those in front of write_below),
        // the block maxima of all other blocks from the streaming kernel
        const bool split = !need && Bmax && write_below < nsrc;
        const int ny = split ? write_below : nsrc;
        if (ny > 0) {
            k_mirror_tiles<<<dim3(ntile, ny), 1024, 128 * MIRROR_PITCH, st>>>(M, ldm, Ic, Bmax, ldb, need, write_below, bpc);
            FY_KERNEL_CHECK();
        }
        if (split) {
            k_colmax_upper<<<dim3(nblk, nsrc - write_below), 1024, 0, st>>>(M, ldm, Ic, Bmax, ldb, write_below, bpc);
            FY_KERNEL_CHECK();
        }
    }
    if (diag) {
        k_mirror_diag<<<nblk, 256, 0, st>>>(M, ldm, Ic, Bmax, ldb);
        FY_KERNEL_CHECK();
    }
}

#include "fy_rm2_kernels.hpp"   // scoring, top-N, branch-and-bound and cooperative-rank kernels (part of this translation unit)
#include "fy_rm2_launch.hpp"    // the kernel selectors and the one launcher per kernel family (part of this translation unit)

static_assert(TOPN_MAX == fy::TOPN_LIST_MAX, "fy_rm2.hpp states the top-N kernels' limit for the other translation units");
static void stray_allow_lds() {   // k_score_stray: (Uc + 1) rater offsets of dynamic LDS, up to 128 KB
    FY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_score_stray), hipFuncAttributeMaxDynamicSharedMemorySize, (STRAY_UCAP + 1) * (int)sizeof(int32_t)));
}

void launch_topn_rows(Context* ctx, hipStream_t st, const float* S, int64_t ldS, int32_t n_cols, int32_t n_rows,
                      const int32_t* n_out, const int32_t* out_off, const int32_t* rank_item_raw, const int32_t* slot2du,
                      const int32_t* uid, int32_t slot0, int32_t aux_value, int32_t* out_user, int32_t* out_item,
                      float* out_score, int32_t* out_aux, int32_t* overflow, int32_t* any_overflow, int32_t top_n_hint) {
    if (n_rows <= 0) return;
    if (!st) st = ctx->stream;
    TopNArgs TA{};
    TA.S = S; TA.ldS = ldS; TA.Ic = n_cols; TA.n_out = n_out; TA.out_off = out_off; TA.rank_item_raw = rank_item_raw; TA.slot2du = slot2du; TA.uid = uid;
    TA.slot_lo = TA.slot0 = slot0;      // n_out / out_off are indexed by (slot - slot_lo): row u reads entry u
    TA.cluster = aux_value; TA.out_user = out_user; TA.out_item = out_item; TA.out_score = out_score; TA.out_cluster = out_aux;
    launch_topn(ctx, st, TA, n_rows, overflow, any_overflow, 0, top_n_hint > TOPN_LONG, top_n_hint, nullptr);
}

}  // namespace fy

// ================================================================ job orchestration
using namespace fy;

// Everything about a job that depends only on the RATINGS and the CLUSTERING (and the rank's share): the CSR / CSC of fy_prep,
// the statistics summed per (cluster, item), and -- filled by the first fy_rm2_score -- the row kernel's tables.  None of it
// depends on lambda, the list length or numberOfItems -- under Jelinek-Mercer.  With a Dirichlet prior or absolute discounting the
// weights x = r' / d_v, b~, the bounds and the tables depend on (method, parameter), which are then part of the key (RM2Static::smooth):
// the structure's csr_r / csc_r hold r', usum_slot holds d_v, b_rank holds b~ (PairPass).  The reference rebuilds all of it in every job (its mappers re-read and
// re-shuffle the ratings, RM2Job.java:130-258); here it is kept on the fy_ratings object (fy_ratings::rm2_cache) and a later
// job over the same ratings and the same clustering starts from it ("warm": fy_stats::prepared_from_cache).  fy_rm2_params::flags
// & FY_RM2_NO_CACHE builds it afresh and does not keep it: the "cold" job, which bench.py times as its headline value.
struct TableCache {
    bool valid = false;
    std::vector<int32_t> sig;           // what the tables were built for: per planned cluster (c, CH, nch, half, panel, p_eff, tail_chunks), + flags
    bool have_x = false;
    DevBuf<float> csc_x, csc_x_over_s;  // x = r / s_v (and x / s_v for the packed walk) per CSC entry: ratings only
    DevBuf<uint32_t> csr_pk, y_pk;      // packed CSR (chunk-relative columns), block-compressed CSR of the tail rows
    DevBuf<int32_t> csc_rank, samples;      // row of every CSC entry; every 64th CSR entry (symmetric cut)
    CsrDescs csr_descs;
    SegStore store;                     // the segment tables of all planned clusters; store.n_seg = fy_stats::cooc_segments
    std::vector<SegTable> segs, segs_tail;      // [plan]: views into it (main walk; tail-row bounds of panel mode)
};
struct RM2Static {
    // key
    int32_t K = 0, rank = 0, world = 1;
    int32_t max_item = -1;      // largest raw item id of the ratings (fy_ratings::max_item): the refinement pass maps raw ids to columns by table
    bool has_count = false;
    std::vector<int32_t> map_user, map_cluster, cluster_count;
    Smoothing smooth;           // general smoothing: (method, parameter); Jelinek-Mercer: method 0 and param 0 whatever lambda is
    // general smoothing: beta_v by slot, S2 per cluster, how b~ was formed (SmoothArgs)
    DevBuf<double> beta_slot, s2_cluster;
    double bt_scale = 0.0;
    int32_t bt_by_n = 0;
    // fy_rm2_prepare
    Prepared P;
    int32_t slot_lo = 0, slot_hi = 0;
    DevBuf<double> partial;     // nI + 1 : this rank's exchange buffer
    // sharded prep (fy_prep.hpp: shard_ratings_by_cluster): P holds this rank's clusters alone and the exchange buffer is by raw id
    bool sharded = false;
    int64_t n_raw_users = 0, n_raw_items = 0;
    std::vector<int32_t> owner;         // [cluster] -> rank (world: empty cluster)
    DevBuf<double> partial_raw;         // n_raw_items + 1 + n_raw_users + 1
    int deferred_code = 0;              // a failure only this rank can see (a duplicate rating / clusteringCount mismatch inside an owned
    std::string deferred_msg;           // cluster): it travels with the statistics so that every rank fails instead of waiting for this one
    int64_t exchange_len() const { return sharded ? n_raw_items + 1 + n_raw_users + 1 : (int64_t)P.nI + 1; }
    // per (cluster, item) in rank order, from the one CSC walk of fy_rm2_prepare (k_pair_pass)
    DevBuf<double> b_rank, usum_slot;
    DevBuf<long long> walk_rank;
    DevBuf<int32_t> cnt_rank, deg_slot;
    DevBuf<float> fx_rank;              // 3 per (cluster, item): see PairPass
    std::vector<float> fx_bounds;       // 3 per cluster (host): max sum of weights, max weight, max rating
    double ms_build = 0;
    TableCache tables;
    std::shared_ptr<void> request_state;   // what fy_rm2_score_users builds from the ratings and the clustering alone and keeps (fy_rm2_request.hip)
    bool matches(const fy_rm2_params* prm, int64_t n_map, const int32_t* mu, const int32_t* mc, const int32_t* cc) const {
        if (K != prm->number_of_clusters || rank != prm->rank || world != prm->world || (int64_t)map_user.size() != n_map || has_count != (cc != nullptr)) return false;
        const Smoothing sm = smoothing_of(*prm);
        if (sm.method != smooth.method || (sm.general() && sm.param != smooth.param)) return false;
        if (n_map && (memcmp(map_user.data(), mu, (size_t)n_map * 4) || memcmp(map_cluster.data(), mc, (size_t)n_map * 4))) return false;
        if (cc && memcmp(cluster_count.data(), cc, (size_t)K * 4)) return false;
        return true;
    }
};

struct fy_rm2_job {
    Context* ctx = nullptr;
    fy_rm2_params prm{};
    std::shared_ptr<RM2Static> S;
    // (the static part under the names the job code has always used)
    Prepared& P;
    int32_t &slot_lo, &slot_hi;
    DevBuf<double>& partial;
    DevBuf<double> stats;       // nI + 1 : global sums (+ counter)
    DevBuf<double> stats_raw;   // sharded prep: the sum over ranks of the raw-id exchange buffers
    bool have_global = false;
    double ms_prepare = 0;
    bool from_cache = false;
    fy_collectives coll{};      // process-group collectives (optional)
    bool have_coll = false;
    DevBuf<double> gathered;    // world * (nI + 1): the statistics all-gathered by fy_rm2_score itself
    DevBuf<double>&b_rank, &usum_slot;
    DevBuf<long long>& walk_rank;
    DevBuf<int32_t>&cnt_rank, &deg_slot;
    DevBuf<float>& fx_rank;
    std::vector<float>& fx_bounds;
    bool count_balanced = false;   // scoring ownership of the users: equal counts instead of equal work (see owner_range)
    SmoothArgs smooth_args() const { return SmoothArgs{S->beta_slot.get(), S->deg_slot.get(), S->s2_cluster.get(), S->bt_scale, S->bt_by_n}; }
    explicit fy_rm2_job(std::shared_ptr<RM2Static> s)
        : S(std::move(s)), P(S->P), slot_lo(S->slot_lo), slot_hi(S->slot_hi), partial(S->partial), b_rank(S->b_rank), usum_slot(S->usum_slot),
          walk_rank(S->walk_rank), cnt_rank(S->cnt_rank), deg_slot(S->deg_slot), fx_rank(S->fx_rank), fx_bounds(S->fx_bounds) {}
};

// Which users does rank k emit lists for?  By default the work-balanced slot range of fy_prep (the rank scores its
// users alone, so equal work).  A single cluster scored cooperatively shares all scoring work anyway and only the top-N
// merge is per owner: equal COUNTS keep the padded reduce-scatter segments small (slots are degree-descending, the
// work-balanced last rank would own four times the average number of users).
static void owner_range(const fy_rm2_job* J, int k, int32_t& lo, int32_t& hi) {
    if (J->S->sharded) { lo = 0; hi = k == J->prm.rank ? J->P.nU : 0; return; }      // this rank's structure holds its own clusters alone
    if (!J->count_balanced) { rank_slot_range(J->P, k, J->prm.world, lo, hi); return; }
    const int64_t n = J->P.nU, W = J->prm.world;
    lo = (int32_t)(n * k / W);
    hi = (int32_t)(n * (k + 1) / W);
}

// launch-shape knobs: fy::Tuning (fy_tuning.hpp), read from the environment ONCE when the context is created
// (fy_context_create / fy_context_reload_tuning in fy_api.hip) -- no job reads the environment.
using ScoreTune = fy::Tuning;

// The upper triangle of the co-rating Gram of a ONE-cluster structure with caller-chosen weights, as fp32 (the item-item
// similarity build, fy_itemsim.hip): G[i][j] = sum_v w_vi r_vj for j > i, zero for (i & ~255) <= j <= i, rows `ldm` floats
// apart; nothing in front of a row's diagonal 256-column block is written.  The same symmetric walk, segment table, item
// list and fixed-point accumulators as the RM2 matrix build -- only the epilogue's scale differs (no (1 - lambda)^2).
// `csc_w` = the weight of every CSC entry (the row side of a product), the column side is the raw rating of the packed
// CSR, or 1 for every entry when `csr_ones` (an array of nnz ones) is given; bounds3 = {largest column sum of the weights, largest
// weight, largest rating} (fx_exponent).  Returns false when the
// fixed-point scale cannot be used (the caller keeps its own path); everything is queued on the context's stream.
bool fy::gram_half_build(Context* ctx, const Prepared& P, const float* csc_w, const float* bounds3, float* G, int64_t ldm, double* ms_tables,
                         double* ms_walk, const float* csr_ones) {
    const ScoreTune tune = ctx->tune;
    const int32_t Ic = P.nP;
    // (csr_ones: both sides of every product are 1 -- exact integers whatever the ratings are)
    if (P.K != 1 || (!csr_ones && (!P.ratings_fp16_exact || !P.ratings_positive)) || Ic <= 0) return false;
    int fxk = fx_exponent(bounds3);
    if (fxk < 0) return false;
    // Ratings that are multiples of 2^-m (half stars: m = 1): every product r r' 2^2m is an integer.  When the largest product
    // stays below 2^24 and the largest possible sum below 2^32 the walk accumulates in 32 bits (ds_add_u32: 6.5 cycles per wave
    // instruction at random addresses against 10.8 for ds_add_u64, profiles/r2/micro_lds_atomic_rate.txt) and a chunk holds
    // twice the columns: two column chunks instead of three at ML-25M shape.  Exact, like the 64-bit sums.
    const int m = csr_ones ? 0 : P.ratings_frac_bits;
    const bool acc32 = tune.isim_acc32 && m <= 4 && (double)bounds3[2] * bounds3[2] * std::ldexp(1.0, 2 * m) < 16777216.0 &&
                       (double)bounds3[0] * bounds3[2] * std::ldexp(1.0, 2 * m) < 4294967296.0;
    if (acc32) fxk = 2 * m;
    int32_t CH, nch;
    pick_chunks(Ic, acc32 && !tune.cooc_max_ch_forced ? 2 * tune.cooc_max_ch : tune.cooc_max_ch, CH, nch);
    if (nch >= 256) return false;                      // (the item ids of the row kernel hold the chunk in 8 bits)
    hipStream_t st = ctx->stream;
    cooc_rm2_allow_lds(tune.cooc_epi);
    EventTimer t_tab(ctx), t_walk(ctx);
    const size_t s0 = t_tab.begin();
    DevBuf<uint32_t> csr_pk(ctx, (size_t)P.nnz);
    DevBuf<int32_t> co(ctx, (size_t)P.nU * (nch + 1)), csc_rank(ctx, (size_t)P.nnz), samples;
    k_csc_rank<<<grid_for(P.nnz), 256, 0, st>>>(P.nnz, P.csc_pair.get(), P.pair_rank.get(), csc_rank.get());
    FY_KERNEL_CHECK();
    build_csr_samples(ctx, P.nnz, P.csr_idx.get(), samples, st);
    const CsrDescs cd = upload_csr_descs(ctx, {csr_desc(0, P.nU, CH, nch, 0, (int32_t)P.nnz)}, st);      // (queued behind the two kernels above)
    pack_csr(ctx, cd, P.csr_idx.get(), csr_ones ? csr_ones : P.csr_r.get(), csr_pk.get(), st);
    build_chunk_offsets(ctx, cd, P.rowptr.get(), P.csr_idx.get(), co.get(), st);
    SegStore segs;
    const SegDesc sd = seg_desc(0, 0, (int32_t)P.nnz, nch, CH, true);
    build_segment_table(ctx, SegArrays{P.csc_slot.get(), csc_w, co.get(), csc_rank.get(), samples.get()}, sd, segs, st);
    CoocArgs CA = cooc_args(P, segs.view(sd), CoocGeometry{0, 0, Ic, CH, nch, 0, (int32_t)P.nnz}, nullptr, csr_pk.get());
    CA.half = 1;
    CA.fx_scale = std::ldexp(1.0, fxk);
    CA.acc32 = acc32 ? 1 : 0;
    const int n_items = (int)cooc_item_count(Ic, CH, nch, true);
    DevBuf<int2> item_seg(ctx, (size_t)Ic * nch);
    DevBuf<int32_t> item_id(ctx, (size_t)Ic * nch), counter(ctx, 1);
    k_item_list<<<grid_for((int64_t)Ic * nch), 256, 0, st>>>(CA, item_seg.get(), item_id.get());
    FY_KERNEL_CHECK();
    CA.item_seg = item_seg.get();
    CA.item_id = item_id.get();
    counter.zero();
    CA.item_grab = cooc_item_grab(P.sum_deg2 / 2, n_items);
    MEpilogue ME{};
    ME.M = G;
    ME.ldm = ldm;
    ME.w2 = 1.0f;
    ME.fx_inv = std::ldexp(1.0, -fxk);
    t_tab.end(s0);
    const size_t s1 = t_walk.begin();
    launch_cooc_rm2(ctx, tune, true, CA, ME, n_items, counter.get(), st);
    t_walk.end(s1);
    sync(ctx);     // the tables of this scope go back to the allocator
    if (ms_tables) *ms_tables = t_tab.total_ms();
    if (ms_walk) *ms_walk = t_walk.total_ms();
    return true;
}

// the host-side plan (fy_rm2_plan.hpp) states the kernels' limits for itself: the two sides must agree
static_assert(PLAN_TOPN_MAX == TOPN_MAX && PLAN_TOPN_SAMPLE == TOPN_SAMPLE && PLAN_TOPN_LONG == TOPN_LONG && PLAN_SEED_CHUNKS_MAX == SEED_CHUNKS_MAX &&
                  PLAN_PRUNE_BLOCK == PRUNE_BLOCK && PLAN_STRAY_UCAP == STRAY_UCAP,
              "fy_rm2_plan.hpp and fy_rm2_kernels.hpp disagree about a limit");

// ================================================================ what the flows of one fy_rm2_score share
// scratch of one lane (a HIP stream the clusters of a job are spread over), or -- two-phase panel mode -- of one cluster
struct Lane {
    hipStream_t st;
    DevBuf<float> M, S;
    DevBuf<int32_t> overflow, any_overflow;
    // branch and bound
    DevBuf<float> Bmax, amax, bmax, UB, tau;
    DevBuf<float> Gp, Bmax64, amax64, bmax64;    // column-panel mode
    DevBuf<uint32_t> Brep;
    DevBuf<uint16_t> surv;
    DevBuf<uint8_t> surv_mask;     // panel mode: which 64-column sub-blocks of a surviving block passed the bound
    DevBuf<int2> strayT;           // co-rater tables of k_score_stray
    DevBuf<int2> stray_items;
    DevBuf<int32_t> n_heavy;       // k_count_heavy
    DevBuf<int32_t> need;          // lazy mirror: column blocks with survivors
    DevBuf<float> Bsup, asup, bsupb, UBs;      // super-block bounds (k_score_sup)
    DevBuf<double> head32, tail32;             // unrounded fp64 rows / columns the refinement pass reads (k_refine_rows)
    DevBuf<int32_t> colmap;
    DevBuf<int32_t> sup_first;
    DevBuf<int32_t> n_quads, quad_prefix;
    DevBuf<char> scan_tmp;         // temporary storage of the lane's scans
    DevBuf<int2> item_seg, item_seg_t;      // (_t: the tail-row bound launch of a cluster whose row kernels are batched)
    DevBuf<int32_t> item_id, item_id_t;
    DevBuf<float> Ssurv;   // packed scores of the surviving blocks (pruned clusters)
};

// the per-job device arrays every flow reads (score_preamble builds them, in this order)
struct JobArrays {
    DevBuf<double> icoll_mine;           // sharded prep: p(i|C) of this rank's own dense items (the result's itemColl is the global one)
    DevBuf<double> d_total;
    DevBuf<double> p_rank;
    DevBuf<float> a_rank, b_rank32;
    DevBuf<double2> pb_rank;
    DevBuf<float> csr_x, csr_e, csr_q;   // per-rating values of the scoring kernels (SideValues)
    DevBuf<float> d_gscale;
    DevBuf<int32_t> d_cshift;
};

// The per-rating values (x, e, q: what the SCORING kernels read): with the packed walk nothing in front of the scoring reads them, and
// what runs until then -- the table kernels, then the one-cluster job's row kernel with ONE workgroup per CU beside its 157 KB of LDS
// accumulators -- leaves wave slots and most of the memory system idle.  They are computed on a side stream; the plain one-cluster
// flow joins behind its row kernel, every other flow (several lanes, cooperative ranks, flat batches) before its lanes start.
class SideValues {
  public:
    explicit SideValues(Context* c) : ctx(c) {}
    SideValues(const SideValues&) = delete;
    SideValues& operator=(const SideValues&) = delete;
    ~SideValues() {     // (a failed job: the side kernel must not outlive the arrays it writes)
        if (!joined && sv) (void)hipStreamSynchronize(sv);
        if (in) (void)hipEventDestroy(in);
        if (out) (void)hipEventDestroy(out);
    }
    // queues k_csr_values behind what `main_stream` holds: on the side stream when `beside` (and FY_OVERLAP_VALUES), else on main_stream
    void launch(hipStream_t main_stream, bool beside, const Prepared& P, double lambda, JobArrays& A, const fy_rm2_job* J) {
        if (launched) return;
        launched = true;
        hipStream_t vs = main_stream;
        if (beside && ctx->tune.overlap_values) {
            if (ctx->aux.empty()) {
                hipStream_t x;
                FY_HIP(hipStreamCreateWithFlags(&x, hipStreamNonBlocking));
                ctx->aux.push_back(x);
            }
            sv = ctx->aux[0];
            FY_HIP(hipEventCreateWithFlags(&in, hipEventDisableTiming));
            FY_HIP(hipEventCreateWithFlags(&out, hipEventDisableTiming));
            FY_HIP(hipEventRecord(in, main_stream));
            FY_HIP(hipStreamWaitEvent(sv, in, 0));
            vs = sv;
        }
        const bool general = J->S->smooth.general();
        (general ? k_csr_values<true> : k_csr_values<false>)<<<grid_for((int64_t)P.nU * 64, 256), 256, 0, vs>>>(
            P.nU, P.rowptr.get(), P.csr_idx.get(), P.csr_r.get(), P.slot2du.get(), P.ucluster.get(), P.usum.get(), P.d_csize.get(), P.d_pcstart.get(),
            A.pb_rank.get(), lambda, A.d_gscale.get(), A.csr_x.get(), A.csr_e.get(), A.csr_q.get(), general ? J->S->usum_slot.get() : nullptr,
            general ? J->smooth_args() : SmoothArgs{});
        FY_KERNEL_CHECK();
        if (vs != main_stream) {
            FY_HIP(hipEventRecord(out, sv));
            joined = false;
        }
    }
    // `s` waits for the values (nothing to do when they were queued on the main stream, or somebody has joined already)
    void join(hipStream_t s) {
        if (joined) return;
        joined = true;
        FY_HIP(hipStreamWaitEvent(s, out, 0));
    }

  private:
    Context* ctx;
    hipStream_t sv = nullptr;
    hipEvent_t in = nullptr, out = nullptr;
    bool launched = false, joined = true;
};

// Read-only view of one job's scoring state: every flow below (and score_cluster_coop, fy_rm2_coop.hpp) receives it by const
// reference.  The device arrays are not written through it; the timers and counters it points to are the job's own.
struct ScoreShared {
    fy_rm2_job* J;
    fy_result* R;
    const ScoreTune* tune;            // the context's knobs, seed_chunks resolved (JobPlan::seed_chunks)
    const JobPlan* jp;
    const float *b_rank;              // b_i (fp32), rank order
    const double *b_rank64, *p_rank;  // b_i and p(i|C) in fp64 (the refinement pass)
    const float *a_rank, *csc_x, *csr_x, *csr_e, *csr_q;
    const uint32_t* csr_pk;        // packed CSR for the row kernel (nullptr: csr_idx / csr_x); csc_x then holds x / s_v
    const int32_t *n_out, *out_off;   // this rank's users, by slot - lo
    const double* pvpi;               // this rank's users, by slot - lo (the complete value; pv_all below is zero on ranks != 0)
    int32_t lo;
    const std::vector<int32_t>* csr_range;     // first / last CSR entry of every planned cluster: [2 * plan], [2 * plan + 1]
    SideValues* side;
    EventTimer *t_cooc, *t_score, *t_topn, *t_mirror;
    unsigned long long* prune_counters;      // [0] surviving blocks, [1] log terms evaluated by the three pruned passes, [2] users sent to k_topn_select, [3] stray blocks (panel mode), [4] bound repairs, [5] list rows scored again by the refinement pass
    int64_t *blocks_total, *seed_terms_cols, *coop_survived, *fallback_survived;
    int64_t* coop_pair_contribs;      // cooperative clusters: ordered off-diagonal co-rating pairs of this rank's matrix rows
    const int32_t* cshift;            // [cluster]: c of the packed matrix format (k_user_meta)
    const float* gscale;              // [cluster], host: 2^-c
};

// Scoring arguments of the users [slot0, slot0 + n_users) of cluster `p` against the matrix M (pitch ldm), scores to S (pitch ldS): the
// job's own CSR and per-rating values.  A second matrix (score_args_bounds), n_heavy, the super-block bounds and the cooperative
// ranks' own CSR are set by member name by the caller.
static ScoreArgs score_args(const ScoreShared& X, const Plan& p, const float* M, int64_t ldm, int32_t slot0, int32_t n_users, float* S, int64_t ldS,
                            int n_slices, int n_chunks) {
    const Prepared& P = X.J->P;
    ScoreArgs SA{};
    SA.M = M; SA.ldm = ldm; SA.Ic = p.Ic; SA.a_rank = X.a_rank + p.pbase; SA.b_rank = X.b_rank + p.pbase;
    SA.rb_off = P.rowptr.get() + p.sbase;     // the users' CSR rows: [slot - sbase], [slot - sbase + 1]
    SA.csr_idx = P.csr_idx.get(); SA.csr_e = X.csr_e; SA.csr_q = X.csr_q;
    SA.pvpi = X.pvpi; SA.n_out = X.n_out; SA.slot_lo = X.lo; SA.slot_base = p.sbase; SA.slot0 = slot0; SA.n_users = n_users;
    SA.S = S; SA.ldS = ldS; SA.n_slices = n_slices; SA.n_chunks = n_chunks;
    return SA;
}
// the fused seed + bound launch: the chunks from `seed_chunks` on work on the block maxima M2 (pitch ld2, n2 columns, the blocks' maxima
// a2 / b2 of a and b), the bounds go to S2 at the same pitch; no "already rated" mask there
static void score_args_bounds(ScoreArgs& SA, int seed_chunks, const float* M2, int64_t ld2, int32_t n2, const float* a2, const float* b2, float* S2) {
    SA.chunks1 = seed_chunks;
    SA.M2 = M2; SA.ldm2 = ld2; SA.Ic2 = n2; SA.a2 = a2; SA.b2 = b2; SA.S2 = S2; SA.ldS2 = ld2; SA.no_mask2 = 1;
}
// Top-N arguments of the users of cluster `p` from slot0 on, score rows S (pitch ldS), lists into the result: mode 0, the whole row is
// live.  The branch and bound sets its fields (topn_pruned) for modes 1 and 2.
static TopNArgs topn_args(const ScoreShared& X, const Plan& p, const float* S, int64_t ldS, int32_t slot0) {
    const Prepared& P = X.J->P;
    TopNArgs TA{};
    TA.S = S; TA.ldS = ldS; TA.Ic = p.Ic; TA.n_out = X.n_out; TA.out_off = X.out_off; TA.rank_item_raw = P.rank_item_raw.get() + p.pbase;
    TA.slot2du = P.slot2du.get(); TA.uid = P.uid.get(); TA.slot_lo = X.lo; TA.slot0 = slot0; TA.cluster = p.c;
    TA.out_user = X.R->d_key0.get(); TA.out_item = X.R->d_key1.get(); TA.out_score = X.R->d_value.get(); TA.out_cluster = X.R->d_aux.get();
    return TA;
}
// mode 1 (seed phase) / mode 2 (merge phase: Ssurv and quad_prefix name the packed scores of the survivors)
static void topn_pruned(TopNArgs& TA, int mode, int32_t seed_cols, const uint16_t* surv, const int32_t* n_quads, int64_t ldb, float* tau,
                        const float* Ssurv = nullptr, const int32_t* quad_prefix = nullptr) {
    TA.mode = mode; TA.seed_cols = seed_cols; TA.surv = surv; TA.n_quads = n_quads; TA.ldb = ldb; TA.tau = tau;
    TA.Ssurv = Ssurv; TA.quad_prefix = quad_prefix;
}

#include "fy_rm2_coop.hpp"   // score_cluster_coop: a cluster scored by all ranks together (part of this translation unit)

static void validate_params(const fy_rm2_params* p) {
    if (!p) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "params is NULL");
    if (p->number_of_clusters <= 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "numberOfClusters must be > 0 (got %d)", p->number_of_clusters);
    if (p->number_of_items <= 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "numberOfItems must be > 0 (got %d)", p->number_of_items);
    const bool dir = p->flags & FY_RM2_SMOOTHING_DIRICHLET, ad = p->flags & FY_RM2_SMOOTHING_ABSOLUTE_DISCOUNT;
    if (dir && ad) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "flags: FY_RM2_SMOOTHING_DIRICHLET and FY_RM2_SMOOTHING_ABSOLUTE_DISCOUNT are both set");
    if (p->flags & ~(FY_RM2_NO_CACHE | FY_RM2_SMOOTHING_DIRICHLET | FY_RM2_SMOOTHING_ABSOLUTE_DISCOUNT | FY_RM2_ESTIMATOR_RM1))
        FY_FAIL(FY_ERR_INVALID_ARGUMENT, "flags: unknown bits 0x%x", p->flags & ~15u);
    if (dir || ad) {
        if (!(std::isfinite(p->lambda) && p->lambda >= 0.0))
            FY_FAIL(FY_ERR_INVALID_ARGUMENT, "%s must be finite and >= 0 (got %g)", dir ? "mu" : "delta", p->lambda);
    } else if (!(p->lambda >= 0.0 && p->lambda <= 1.0)) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "lambda must be in [0, 1]");
    if (p->world <= 0 || p->rank < 0 || p->rank >= p->world) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "rank %d of world %d", p->rank, p->world);
    if (p->number_of_recommendations < 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "numberOfRecommendations must be >= 0");
}

fy_rm2_job* fy::rm2_prepare(Context* ctx, const fy_rm2_params* prm, const fy_ratings* R, int64_t n_map, const int32_t* map_user,
                            const int32_t* map_cluster, const int32_t* cluster_count) {
    validate_params(prm);
    if (n_map < 0 || (n_map > 0 && (!map_user || !map_cluster))) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "clustering map is NULL");
    EventTimer tm(ctx);
    const size_t span = tm.begin();
    const bool use_cache = !(prm->flags & FY_RM2_NO_CACHE);
    if (use_cache) {
        std::shared_ptr<RM2Static> have;
        {
            std::lock_guard<std::mutex> g(R->cache_mu);
            have = std::static_pointer_cast<RM2Static>(R->rm2_cache);
            // another clustering, rank or world: the old static set (CSR / CSC, statistics, every table of the row kernel) goes back to
            // the allocator BEFORE the new one is built -- peak HBM is one set plus the job's scratch, not two
            if (have && !have->matches(prm, n_map, map_user, map_cluster, cluster_count)) { R->rm2_cache.reset(); have.reset(); }
        }
        if (have) {      // warm: same ratings, same clustering, same share
            std::unique_ptr<fy_rm2_job> J(new fy_rm2_job(have));
            J->ctx = ctx;
            J->prm = *prm;
            J->from_cache = true;
            tm.end(span);
            sync(ctx);
            J->ms_prepare = tm.total_ms();
            return J.release();
        }
    }
    std::shared_ptr<RM2Static> fresh = std::make_shared<RM2Static>();
    fresh->K = prm->number_of_clusters;
    fresh->rank = prm->rank;
    fresh->world = prm->world;
    fresh->max_item = R->max_item;
    fresh->has_count = cluster_count != nullptr;
    {
        const Smoothing sm = smoothing_of(*prm);
        fresh->smooth.method = sm.method;
        fresh->smooth.param = sm.general() ? sm.param : 0.0;
    }
    if (n_map) { fresh->map_user.assign(map_user, map_user + n_map); fresh->map_cluster.assign(map_cluster, map_cluster + n_map); }
    if (cluster_count) fresh->cluster_count.assign(cluster_count, cluster_count + prm->number_of_clusters);
    std::unique_ptr<fy_rm2_job> J(new fy_rm2_job(fresh));
    J->ctx = ctx;
    J->prm = *prm;
    // Several ranks and at least as many clusters as ranks: this rank preps the ratings of its own clusters alone (the reference's
    // map-side partitioning by cluster, IntKeyPartitioner.java:15); the statistics are then exchanged by raw id.
    fy_ratings mine;
    DevBuf<int32_t> cl_table;
    SyncOnUnwind mine_guard(ctx->stream);       // (a failure below must not free `mine` under a queued kernel)
    RM2Static& S = *fresh;
    if (prm->world > 1 && ctx->tune.shard_prep)
        S.sharded = shard_ratings_by_cluster(ctx, R, prm->number_of_clusters, n_map, map_user, map_cluster, prm->rank, prm->world, mine, S.owner, cl_table);
    Prepared& P = J->P;
    if (S.sharded) {
        S.n_raw_users = (int64_t)R->max_user + 1;
        S.n_raw_items = (int64_t)R->max_item + 1;
        S.partial_raw.alloc(ctx, (size_t)S.exchange_len());
        S.partial_raw.zero();
        try {
            build_structure(ctx, &mine, prm->number_of_clusters, n_map, map_user, map_cluster, cluster_count, false, J->P, cl_table.get());
        } catch (const Failure& f) {
            if (f.code != FY_ERR_DUPLICATE_RATING && f.code != FY_ERR_CLUSTER_COUNT) throw;
            // only this rank's share shows it: the other ranks learn of it from the flag at the end of the exchange buffer
            // (fy_rm2_set_global_stats fails on EVERY rank then, none waits in a collective for a rank that has gone)
            S.deferred_code = f.code;
            S.deferred_msg = last_error();
            const double flag = (double)(-f.code);
            sync(ctx);
            FY_HIP(hipMemcpyAsync(S.partial_raw.get() + (S.exchange_len() - 1), &flag, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            tm.end(span);
            sync(ctx);
            J->ms_prepare = tm.total_ms();
            return J.release();
        }
        J->slot_lo = 0;
        J->slot_hi = P.nU;
    } else {
        build_structure(ctx, R, prm->number_of_clusters, n_map, map_user, map_cluster, cluster_count, false, J->P);
        rank_slot_range(P, prm->rank, prm->world, J->slot_lo, J->slot_hi);
    }
    J->partial.alloc(ctx, (size_t)P.nI + 1);
    J->partial.zero();
    // (sharded: the raw-id copy of the exchange buffer, queued behind the kernels that fill `partial` below)
    auto publish_raw = [&]() {
        if (!S.sharded) return;
        const int32_t n = std::max(P.nI + 1, P.nU);
        k_stats_to_raw<<<grid_for(n), 256, 0, ctx->stream>>>(P.nI, P.iid.get(), J->partial.get(), S.n_raw_items, P.nU, P.uid.get(), P.usum.get(),
                                                              S.partial_raw.get());
        FY_KERNEL_CHECK();
    };
    if (P.nnz > 0) {
        DevBuf<unsigned long long> counter(ctx, 1);
        counter.zero();
        J->usum_slot.alloc(ctx, (size_t)P.nU);
        J->deg_slot.alloc(ctx, (size_t)P.nU);
        DevBuf<double2> ud_slot(ctx, (size_t)P.nU);
        const Smoothing sm = S.smooth;
        const double delta = sm.method == 2 ? sm.param : 0.0;
        if (sm.general()) {
            S.beta_slot.alloc(ctx, (size_t)P.nU);
            S.s2_cluster.alloc(ctx, (size_t)P.K);
            S.bt_scale = sm.param;
            S.bt_by_n = sm.method == 2 ? 1 : 0;
            k_slot_user_arrays_gen<<<grid_for(P.nU), 256, 0, ctx->stream>>>(P.nU, P.slot2du.get(), P.usum.get(), P.udeg.get(), sm.method, sm.param,
                                                                            J->usum_slot.get(), J->deg_slot.get(), ud_slot.get(), S.beta_slot.get());
            FY_KERNEL_CHECK();
            k_cluster_s2<<<(unsigned)P.K, 256, 0, ctx->stream>>>(P.d_ucstart.get(), S.beta_slot.get(), S.s2_cluster.get());
            FY_KERNEL_CHECK();
            if (delta > 0.0) {      // the packed walk needs r' (not r) exactly representable in fp16
                DevBuf<int32_t> d_flag(ctx, 1);
                d_flag.zero();
                k_discount_not_fp16<<<grid_for(P.nnz), 256, 0, ctx->stream>>>(P.nnz, delta, P.csc_r.get(), d_flag.get());
                FY_KERNEL_CHECK();
                int32_t flag = 0;
                d2h(ctx, &flag, d_flag.get(), 1);
                sync(ctx);
                P.ratings_fp16_exact = flag == 0;
                P.ratings_positive = false;      // (r <= delta leaves r' = 0)
            }
        } else {
            k_slot_user_arrays<<<grid_for(P.nU), 256, 0, ctx->stream>>>(P.nU, P.slot2du.get(), P.usum.get(), P.udeg.get(), J->usum_slot.get(),
                                                                        J->deg_slot.get(), ud_slot.get());
            FY_KERNEL_CHECK();
        }
        // the walk's per-rating weights are written by the statistics pass (same gather): x / s_v for the packed walk, x for the plain one
        TableCache& tc0 = S.tables;
        const bool use_pk0 = ctx->tune.cooc_pk && P.ratings_fp16_exact;
        tc0.csc_x.alloc(ctx, (size_t)P.nnz);      // (x itself is also what the stray blocks of the panel mode are scored from)
        tc0.csc_x_over_s.alloc(ctx, use_pk0 ? (size_t)P.nnz : 1);
        tc0.have_x = true;
        J->b_rank.alloc(ctx, (size_t)P.nP);
        J->walk_rank.alloc(ctx, (size_t)P.nP);
        J->cnt_rank.alloc(ctx, (size_t)P.nP);
        J->fx_rank.alloc(ctx, 3 * (size_t)P.nP);
        // heavy columns (more than PAIR_HEAVY raters): at most nnz / PAIR_HEAVY of them, at most nnz / PAIR_HEAVY chunks
        const size_t max_heavy = (size_t)(P.nnz / PAIR_HEAVY) + 1;
        DevBuf<int32_t> heavy_col(ctx, max_heavy), heavy_base(ctx, max_heavy), chunk_col(ctx, max_heavy), heavy_counters(ctx, 2);
        DevBuf<PairAcc> chunk_acc(ctx, max_heavy);
        heavy_counters.zero();
        const PairPass PA{P.rank_pair.get(), P.pair_start.get(), P.pair_di.get(), P.csc_slot.get(), P.csc_r.get(), ud_slot.get(), J->slot_lo, J->slot_hi,
                          tc0.csc_x.get(), use_pk0 ? tc0.csc_x_over_s.get() : nullptr,
                          J->partial.get(), J->b_rank.get(), J->walk_rank.get(), J->cnt_rank.get(), J->fx_rank.get(),
                          delta, S.bt_scale, S.bt_by_n};
        const PairHeavy PH{heavy_col.get(), heavy_base.get(), chunk_col.get(), heavy_counters.get(), chunk_acc.get()};
        const unsigned g_chunks = (unsigned)std::min<size_t>(max_heavy, (size_t)ctx->num_cus * 32);
        const unsigned g_finish = (unsigned)std::min<size_t>(ceil_div((int64_t)max_heavy, 64), 1024);
        const bool gen = sm.general(), narrow = P.nnz < 24 * (int64_t)P.nP;      // (narrow: 16 lanes per column instead of a wave)
        (gen ? (narrow ? k_pair_pass<16, true> : k_pair_pass<64, true>) : (narrow ? k_pair_pass<16, false> : k_pair_pass<64, false>))
            <<<grid_for((int64_t)P.nP * (narrow ? 16 : 64), 256), 256, 0, ctx->stream>>>(P.nP, PA, PH);
        FY_KERNEL_CHECK();
        (gen ? k_pair_chunks<true> : k_pair_chunks<false>)<<<g_chunks, 256, 0, ctx->stream>>>(PA, PH);
        FY_KERNEL_CHECK();
        (gen ? k_pair_finish<true> : k_pair_finish<false>)<<<g_finish, 64, 0, ctx->stream>>>(PA, PH);
        FY_KERNEL_CHECK();
        if (gen && delta > 0.0) {      // from here on the structure holds r'
            k_discount_inplace<<<grid_for(P.nnz), 256, 0, ctx->stream>>>(P.nnz, delta, P.csr_r.get(), P.csc_r.get());
            FY_KERNEL_CHECK();
        }
        if (J->slot_hi > J->slot_lo) {
            k_partial_total<<<grid_for(J->slot_hi - J->slot_lo), 256, 0, ctx->stream>>>(J->slot_lo, J->slot_hi, P.slot2du.get(),
                                                                                         P.usum.get(), counter.get());
            FY_KERNEL_CHECK();
        }
        k_store_total<<<1, 1, 0, ctx->stream>>>(counter.get(), J->partial.get() + P.nI);
        FY_KERNEL_CHECK();
        publish_raw();
        DevBuf<float> d_fx(ctx, 3 * (size_t)P.K);
        d_fx.zero();
        k_cluster_fx_bounds<<<dim3((unsigned)P.K, (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (int64_t)P.nP / ((int64_t)P.K * 1024)))), 256, 0, ctx->stream>>>(
            P.d_pcstart.get(), J->fx_rank.get(), d_fx.get());
        FY_KERNEL_CHECK();
        J->fx_bounds.resize(3 * (size_t)P.K);
        d2h(ctx, J->fx_bounds.data(), d_fx.get(), 3 * (size_t)P.K);
        tm.end(span);
        sync(ctx);
        J->ms_prepare = tm.total_ms();
        if (use_cache) { std::lock_guard<std::mutex> g(R->cache_mu); R->rm2_cache = fresh; }
        return J.release();
    }
    tm.end(span);
    sync(ctx);
    J->ms_prepare = tm.total_ms();
    if (use_cache) { std::lock_guard<std::mutex> g(R->cache_mu); R->rm2_cache = fresh; }
    return J.release();
}

void fy::rm2_set_global_stats(fy_rm2_job* J, const double* gathered, int32_t world) {
    Context* ctx = J->ctx;
    if (world != J->prm.world) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "gathered world %d != params.world %d", world, J->prm.world);
    const RM2Static& S = *J->S;
    const int64_t len = S.exchange_len();
    if (S.sharded) {
        if (world > 1024) FY_FAIL(FY_ERR_UNSUPPORTED, "more than 1024 ranks");
        // did any rank's share fail?  (the flags are read before anything is built from the sums)
        DevBuf<double> d_flags(ctx, (size_t)world);
        k_rank_flags<<<1, 1024, 0, ctx->stream>>>(world, len, gathered, d_flags.get());
        FY_KERNEL_CHECK();
        std::vector<double> flags((size_t)world);
        d2h(ctx, flags.data(), d_flags.get(), (size_t)world);
        sync(ctx);
        if (S.deferred_code) { set_error("%s", S.deferred_msg.c_str()); throw Failure{S.deferred_code}; }
        for (int r = 0; r < world; r++)
            if (flags[(size_t)r] != 0.0) {
                const int code = -(int)flags[(size_t)r];
                FY_FAIL(code, "rank %d found %s in the clusters it owns", r,
                        code == FY_ERR_DUPLICATE_RATING ? "two ratings with one (user, item) key" : "a clusteringCount that disagrees with the rated users");
            }
        J->stats_raw.alloc(ctx, (size_t)len);
        k_sum_gathered<<<grid_for(len), 256, 0, ctx->stream>>>(len, world, gathered, J->stats_raw.get());
        FY_KERNEL_CHECK();
        J->stats.alloc(ctx, (size_t)J->P.nI + 1);
        k_stats_from_raw<<<grid_for((int64_t)J->P.nI + 1), 256, 0, ctx->stream>>>(J->P.nI, J->P.iid.get(), J->stats_raw.get(), S.n_raw_items, J->stats.get());
        FY_KERNEL_CHECK();
        J->have_global = true;
        return;
    }
    J->stats.alloc(ctx, (size_t)len);
    k_sum_gathered<<<grid_for(len), 256, 0, ctx->stream>>>(len, world, gathered, J->stats.get());
    FY_KERNEL_CHECK();
    J->have_global = true;
}

// Sharded prep: the result's side outputs are the GLOBAL statistics (jobs RM2-1 / RM2-2 write one userSum and one itemColl for all clusters),
// compacted out of the summed raw-id exchange buffer -- on every rank, whatever it prepared or scored (include/filmyou.h).
static void sharded_side_outputs(fy_rm2_job* J, fy_result* R, const double* d_total) {
    Context* ctx = J->ctx;
    hipStream_t st = ctx->stream;
    const RM2Static& S = *J->S;
    const double* raw_items = J->stats_raw.get();
    const double* raw_users = J->stats_raw.get() + S.n_raw_items + 1;
    DevBuf<uint32_t> fi(ctx, (size_t)S.n_raw_items), pi(ctx, (size_t)S.n_raw_items), fu(ctx, (size_t)S.n_raw_users), pu(ctx, (size_t)S.n_raw_users);
    k_flag_positive<<<grid_for(S.n_raw_items), 256, 0, st>>>(S.n_raw_items, raw_items, fi.get());
    FY_KERNEL_CHECK();
    k_flag_positive<<<grid_for(S.n_raw_users), 256, 0, st>>>(S.n_raw_users, raw_users, fu.get());
    FY_KERNEL_CHECK();
    inclusive_scan_u32(ctx, fi.get(), pi.get(), (size_t)S.n_raw_items);
    inclusive_scan_u32(ctx, fu.get(), pu.get(), (size_t)S.n_raw_users);
    uint32_t n_items_all = 0, n_users_all = 0;
    d2h(ctx, &n_items_all, pi.get() + (S.n_raw_items - 1), 1);
    d2h(ctx, &n_users_all, pu.get() + (S.n_raw_users - 1), 1);
    sync(ctx);
    R->d_item_id.alloc(ctx, n_items_all);
    R->d_icoll.alloc(ctx, n_items_all);
    R->d_user_id.alloc(ctx, n_users_all);
    R->d_user_sum.alloc(ctx, n_users_all);
    k_compact_positive<<<grid_for(S.n_raw_items), 256, 0, st>>>(S.n_raw_items, raw_items, pi.get(), d_total, R->d_item_id.get(), R->d_icoll.get());
    FY_KERNEL_CHECK();
    k_compact_positive<<<grid_for(S.n_raw_users), 256, 0, st>>>(S.n_raw_users, raw_users, pu.get(), nullptr, R->d_user_id.get(), R->d_user_sum.get());
    FY_KERNEL_CHECK();
    R->st.n_users = n_users_all;
    R->st.n_items = n_items_all;
    sync(ctx);      // (the flags and positions are released here)
}

// ================================================================ fy_rm2_score: one function per flow, in the order they run
// (fy::rm2_score at the end of this section is the sequence; what to run is decided by plan_job, fy_rm2_plan.hpp)

// ---- 1. p(i|C), per-(cluster,item) statistics, per-rating values
// (sharded prep: the job's own dense items are this rank's clusters' items; the result's itemColl is the global one, built at the end)
static void score_preamble(fy_rm2_job* J, fy_result* R, const PackPlan& pack, bool use_pk, JobArrays& A, SideValues& side) {
    Context* ctx = J->ctx;
    const Prepared& P = J->P;
    hipStream_t st = ctx->stream;
    const int32_t nP = P.nP, nI = P.nI, K = P.K;
    const double lambda = J->prm.lambda;
    if (J->S->sharded) A.icoll_mine.alloc(ctx, nI); else R->d_icoll.alloc(ctx, nI);
    double* const d_icoll = J->S->sharded ? A.icoll_mine.get() : R->d_icoll.get();
    A.d_total.alloc(ctx, 1);
    k_item_coll<<<grid_for(nI), 256, 0, st>>>(nI, J->stats.get(), d_icoll, A.d_total.get());
    FY_KERNEL_CHECK();
    A.p_rank.alloc(ctx, nP);
    A.a_rank.alloc(ctx, nP);
    A.b_rank32.alloc(ctx, nP);
    A.pb_rank.alloc(ctx, nP);
    (J->S->smooth.general() ? k_pair_p<true> : k_pair_p<false>)<<<grid_for(nP), 256, 0, st>>>(nP, P.rank_pair.get(), P.pair_di.get(), d_icoll, lambda, J->b_rank.get(),
                                                                                            A.p_rank.get(), A.a_rank.get(), A.b_rank32.get(), A.pb_rank.get());
    FY_KERNEL_CHECK();
    A.csr_x.alloc(ctx, P.nnz);
    A.csr_e.alloc(ctx, P.nnz);
    A.csr_q.alloc(ctx, P.nnz);
    // the row kernel's tables live with the static part of the job (TableCache): a warm job finds them built
    TableCache& tc = J->S->tables;
    // (normally written by fy_rm2_prepare's statistics pass; here only when the walk's kind changed between the two calls)
    if (!tc.have_x || tc.csc_x.size() != (size_t)P.nnz || tc.csc_x_over_s.size() != (use_pk ? (size_t)P.nnz : 1)) {
        tc.valid = tc.have_x = false;
        tc.csc_x.alloc(ctx, P.nnz);
        tc.csc_x_over_s.alloc(ctx, use_pk ? (size_t)P.nnz : 1);
        k_csc_x<<<grid_for(P.nnz), 256, 0, st>>>(P.nnz, P.csc_slot.get(), P.csc_r.get(), J->usum_slot.get(), tc.csc_x.get(),
                                                 use_pk ? tc.csc_x_over_s.get() : nullptr);
        FY_KERNEL_CHECK();
        tc.have_x = true;
    }
    // (which clusters keep packed 24-bit rows, and their scales 2^-c: plan_pack24)
    A.d_gscale.alloc(ctx, (size_t)K);
    A.d_cshift.alloc(ctx, (size_t)K);
    h2d(ctx, A.d_gscale.get(), pack.h_gscale.data(), (size_t)K);
    h2d(ctx, A.d_cshift.get(), pack.h_cshift.data(), (size_t)K);
    // (the packed walk reads the packed CSR; the PLAIN walk's row kernel reads x itself: no overlap there.  Measured on one box, ML-25M
    // shape, ms per cold job: side stream from here 20.08, launched right in front of the row kernel 20.15, main stream 20.30 / 20.48 --
    // the table kernels in between wait on the L2's request rate and on dependent loads, and leave more room than the row kernel.)
    side.launch(st, use_pk, P, lambda, A, J);
}

// ---- 2. per-user meta for this rank's slots [lo, hi), output offsets; returns the number of list entries the rank emits
struct UserMeta {
    DevBuf<double> pvpi;
    DevBuf<int32_t> n_out, out_off;
    DevBuf<unsigned long long> counters;
};
static int64_t user_meta_and_offsets(fy_rm2_job* J, fy_result* R, int32_t lo, int32_t hi, const int32_t* d_cshift, UserMeta& U) {
    Context* ctx = J->ctx;
    const Prepared& P = J->P;
    const fy_rm2_params& prm = J->prm;
    hipStream_t st = ctx->stream;
    const int32_t nmine = hi - lo;
    U.pvpi.alloc(ctx, (size_t)nmine + 1);
    U.n_out.alloc(ctx, (size_t)nmine + 1);
    U.out_off.alloc(ctx, (size_t)nmine + 1);
    U.counters.alloc(ctx, 2);
    U.counters.zero();
    U.n_out.zero();
    if (nmine > 0) {
        k_user_meta<<<grid_for(nmine), 256, 0, st>>>(lo, hi, P.slot2du.get(), P.uid.get(), P.ucluster.get(), P.udeg.get(),
                                                      P.d_csize.get(), P.d_pcstart.get(), prm.number_of_items,
                                                      prm.number_of_recommendations, prm.filter_users, d_cshift, U.pvpi.get(), U.n_out.get(), U.counters.get());
        FY_KERNEL_CHECK();
    }
    exclusive_scan_i32(ctx, U.n_out.get(), U.out_off.get(), (size_t)nmine + 1);
    const int64_t n_recs = fetch(ctx, U.out_off.get() + nmine);
    {
        unsigned long long hc[2];
        d2h(ctx, hc, U.counters.get(), 2);
        sync(ctx);
        R->st.log_terms = (int64_t)hc[0];
        R->st.users_scored = (int64_t)hc[1];
    }
    R->n = n_recs;
    R->st.recs = n_recs;
    R->d_key0.alloc(ctx, (size_t)n_recs);
    R->d_key1.alloc(ctx, (size_t)n_recs);
    R->d_value.alloc(ctx, (size_t)n_recs);
    R->d_aux.alloc(ctx, (size_t)n_recs);
    return n_recs;
}

// ---- 3. the lanes' streams and scratch, sized by the plan (JobPlan::*_el)
static void alloc_lanes(Context* ctx, const JobPlan& jp, std::vector<Lane>& lanes) {
    hipStream_t st = ctx->stream;
    const int NS = jp.NS;
    const bool two_phase = jp.two_phase;
    const size_t m_el = jp.m_el, s_el = jp.s_el, ov_el = jp.ov_el, bm_el = jp.bm_el, ub_el = jp.ub_el, am_el = jp.am_el, gp_el = jp.gp_el, b64_el = jp.b64_el,
                 a64_el = jp.a64_el, is_el = jp.is_el;
    if (NS > 1 && ctx->aux.size() < (size_t)NS) {
        while (ctx->aux.size() < (size_t)NS) {
            hipStream_t x;
            FY_HIP(hipStreamCreateWithFlags(&x, hipStreamNonBlocking));
            ctx->aux.push_back(x);
        }
    }
    for (int l = 0; l < NS; l++) {
        Lane& L = lanes[l];
        L.st = NS > 1 ? ctx->aux[l] : st;
        L.M.alloc(ctx, m_el);
        L.S.alloc(ctx, s_el);
        L.overflow.alloc(ctx, ov_el);
        L.any_overflow.alloc(ctx, 1);
        L.n_heavy.alloc(ctx, 1);
        L.Bmax.alloc(ctx, bm_el);
        L.amax.alloc(ctx, am_el);
        L.bmax.alloc(ctx, am_el);
        L.Gp.alloc(ctx, two_phase ? 1 : gp_el);
        L.Bmax64.alloc(ctx, two_phase ? 1 : b64_el);
        L.Brep.alloc(ctx, gp_el > 1 && !two_phase ? b64_el * 4 / 3 + 4 : 1);     // (b64_el counts floats for 3-byte entries)
        L.amax64.alloc(ctx, two_phase ? 1 : a64_el);
        L.bmax64.alloc(ctx, two_phase ? 1 : a64_el);
        L.UB.alloc(ctx, ub_el);
        L.tau.alloc(ctx, ov_el);
        L.surv.alloc(ctx, ub_el);
        L.surv_mask.alloc(ctx, gp_el > 1 ? ub_el : 1);
        L.n_quads.alloc(ctx, ov_el + 1);
        L.quad_prefix.alloc(ctx, ov_el + 1);
        L.item_seg.alloc(ctx, is_el);
        L.item_id.alloc(ctx, is_el);
    }
}

// ---- 4. the row kernel's tables: kept with the job's static part -- a job over the same ratings, clustering and launch plan
// (the signature) re-uses them
static std::vector<int32_t> table_signature(const JobPlan& jp) {
    const std::vector<Plan>& plans = jp.plans;
    std::vector<int32_t> sig;
    sig.push_back(jp.use_pk ? 1 : 0);
    sig.push_back(1);      // (one layout over all planned clusters, whatever their number)
    for (auto& p : plans) {
        const int32_t v[8] = {p.c, p.CH, p.nch, p.half ? 1 : 0, p.panel ? 1 : 0, p.p_eff, p.tail_chunks, (p.coop ? 1 : 0) | (p.flat ? 2 : 0) | (p.psym ? 4 : 0) | (p.rect ? 8 : 0)};
        sig.insert(sig.end(), v, v + 8);
    }
    return sig;
}

// Everything the row kernels of the plan need, on the main stream before the lanes fork; nothing when a job with the same signature
// has left them (`tables_cached`).  Fills csr_range.  The tables of ALL planned clusters are built in one pass over the CSR / CSC
// (layout_tables, fy_rm2_tables.hpp): packed CSR and chunk offsets of every cluster, the tail rows' block-compressed CSR, and both
// segment tables (main walk; tail-row bounds) of every cluster as ranges of ONE store -- one count launch per group, ONE scan, one
// host round trip for the size, one fill.  A cooperative cluster gets its packed CSR here; its ranks build the tables of their own
// rows (coop_build_rows).  (Building cluster by cluster cost a host round trip per table: 20 ms at 50 clusters.)
static void build_job_tables(fy_rm2_job* J, const JobPlan& jp, bool tables_cached, std::vector<int32_t>& csr_range) {
    Context* ctx = J->ctx;
    const Prepared& P = J->P;
    hipStream_t st = ctx->stream;
    TableCache& tc = J->S->tables;
    const std::vector<Plan>& plans = jp.plans;
    // first / last CSR entry of every planned cluster (slots are cluster-major): one round trip for all of them
    csr_range.assign(2 * plans.size() + 2, 0);
    {
        std::vector<int32_t> where(2 * plans.size());
        for (size_t pi = 0; pi < plans.size(); pi++) {
            where[2 * pi] = plans[pi].sbase;
            where[2 * pi + 1] = plans[pi].sbase + plans[pi].Uc;
        }
        gather_to_host_i32(ctx, P.rowptr.get(), where, csr_range.data());
    }
    if (tables_cached) return;
    tc.valid = false;
    tc.csr_pk.alloc(ctx, jp.use_pk ? (size_t)P.nnz : 1);
    tc.y_pk.alloc(ctx, jp.any_tail ? (size_t)P.nnz : 1);     // k_tail_blocks
    tc.csc_rank.alloc(ctx, jp.any_half ? (size_t)P.nnz : 1);     // row (rank inside its cluster) of every CSC entry
    if (jp.any_half) {      // (queued behind the round trip above and in front of the descriptors' upload, which hides behind them on the idle stream)
        k_csc_rank<<<grid_for(P.nnz), 256, 0, st>>>(P.nnz, P.csc_pair.get(), P.pair_rank.get(), tc.csc_rank.get());
        FY_KERNEL_CHECK();
        build_csr_samples(ctx, P.nnz, P.csr_idx.get(), tc.samples, st);
    }
    TableLayout L;
    try {
        L = layout_tables(plans, csr_range);
    } catch (const PlanError& e) {
        FY_FAIL(e.code, "%s", e.msg.c_str());
    }
    const size_t np = plans.size();
    DevBuf<int32_t> co(ctx, (size_t)std::max<int64_t>(1, L.co_total)), co_tail(ctx, (size_t)std::max<int64_t>(1, L.co_tail_total));
    tc.csr_descs = upload_csr_descs(ctx, L.csr, st);      // (kept with the tables: a job without a table of its own has no closing synchronisation)
    const CsrDescs& cd = tc.csr_descs;
    if (jp.use_pk) pack_csr(ctx, cd, P.csr_idx.get(), P.csr_r.get(), tc.csr_pk.get(), st);
    build_chunk_offsets(ctx, cd, P.rowptr.get(), P.csr_idx.get(), co.get(), st);
    if (L.co_tail_total > 0) {
        int32_t max_slots = 1;
        for (auto& d : L.csr) max_slots = std::max(max_slots, d.n_slots);
        k_tail_blocks<<<dim3((unsigned)std::min<int>(max_slots, ctx->num_cus * (np == 1 ? 16 : 4)), (unsigned)np), 256, 0, st>>>(cd.d.get(), P.rowptr.get(), P.csr_idx.get(),
                                                                                                                     P.csr_r.get(), tc.y_pk.get(), co_tail.get());
        FY_KERNEL_CHECK();
    }
    // main tables read co, tail tables co_tail (their "chunk offsets" are the k_tail_blocks ranges): two groups of one build
    const SegGroup groups[2] = {
        {SegArrays{P.csc_slot.get(), jp.use_pk ? tc.csc_x_over_s.get() : tc.csc_x.get(), co.get(), tc.csc_rank.get(), tc.samples.get()}, L.seg.data(), L.n_main},
        {SegArrays{P.csc_slot.get(), tc.csc_x_over_s.get(), co_tail.get(), tc.csc_rank.get(), tc.samples.get()}, L.seg.data() + L.n_main, L.seg.size() - L.n_main}};
    build_segment_tables(ctx, groups, 2, tc.store, st);
    tc.segs.assign(np, SegTable{});
    tc.segs_tail.assign(np, SegTable{});
    for (size_t pi = 0; pi < np; pi++) {
        if (L.main_of[pi] >= 0) tc.segs[pi] = tc.store.view(L.seg[(size_t)L.main_of[pi]]);
        if (L.tail_of[pi] >= 0) tc.segs_tail[pi] = tc.store.view(L.seg[(size_t)L.tail_of[pi]]);
    }
}

// ---- 5. flat batch (Plan::flat): matrix build, scores and lists of all those clusters, one launch per kernel, on the main stream
struct FlatBuffers {      // (kept by fy_rm2_score until the job has drained)
    DevBuf<char> flatM;
    DevBuf<float> flatS;
    DevBuf<int2> flat_seg;
    DevBuf<int32_t> flat_id, flat_ov, flat_flags, flat_cnt;
    DevBuf<CoocLaunch> d_flat_launch;
    DevBuf<FlatDesc> d_flat[2];
};
static void score_flat_batches(const ScoreShared& X, FlatBuffers& F) {
    fy_rm2_job* J = X.J;
    Context* ctx = X.J->ctx;
    const Prepared& P = X.J->P;
    fy_result* R = X.R;
    const ScoreTune& tune = *X.tune;
    const JobPlan& jp = *X.jp;
    hipStream_t st = ctx->stream;
    TableCache& tc = J->S->tables;
    const double lambda = J->prm.lambda;
    constexpr int VEC = 4;   // floats per lane of the scoring kernel: column chunk = 256 items
    for (size_t first = 0; first < jp.plans.size();) {
        std::vector<CoocLaunch> fb;
        std::vector<FlatDesc> fd[2];       // [0] fp32 rows, [1] 24-bit rows
        SyncOnUnwind fb_fd_guard(st);      // (their uploads are queued below; the batch's own synchronisation is at its end)
        size_t m_bytes = 0, s_el = 0, i_el = 0, u_el = 0, n_flat = 0, last = first;
        int64_t batch_bytes = 0;
        for (; last < jp.plans.size(); last++) {
            const Plan& p = jp.plans[last];
            if (!p.flat) continue;
            if (n_flat && batch_bytes + flat_need(p) > jp.flat_budget) break;
            batch_bytes += flat_need(p);
            m_bytes += round_up((int64_t)p.Ic * p.ldm * (p.pack24 ? 3 : 4), 256);
            s_el += (size_t)(p.b - p.a) * p.ldm;
            i_el += (size_t)p.Ic * p.nch;
            u_el += (size_t)(p.b - p.a);
            n_flat++;
        }
        if (n_flat) {
            F.flatM.alloc(ctx, m_bytes);
            F.flatS.alloc(ctx, s_el);
            F.flat_seg.alloc(ctx, i_el);
            F.flat_id.alloc(ctx, i_el);
            F.flat_ov.alloc(ctx, u_el);
            F.flat_flags.alloc(ctx, 2 * n_flat);       // per cluster: n_heavy, any_overflow
            size_t m_at = 0, s_at = 0, i_at = 0, u_at = 0, k = 0;
            int max_grid[2] = {0, 0}, max_users[2] = {0, 0};
            for (size_t pi = first; pi < last; pi++) {
                const Plan& p = jp.plans[pi];
                if (!p.flat) continue;
                const int c = p.c;
                const int32_t nb = p.b - p.a;
                float* const Mc = reinterpret_cast<float*>(F.flatM.get() + m_at);
                float* const Sc = F.flatS.get() + s_at;
                CoocArgs CA = cooc_args(P, tc.segs[pi], cooc_geometry(p), X.csr_x, X.csr_pk);
                const int fxk = fx_exponent(&J->fx_bounds[3 * (size_t)c]);
                CA.fx_scale = std::ldexp(1.0, fxk);
                const double w2s = J->S->smooth.w2_of(lambda) * (double)X.gscale[(size_t)c];
                MEpilogue ME{Mc, p.ldm, (float)w2s, std::ldexp(w2s, -fxk), p.pack24 ? 1 : 0, nullptr, p.ldb, 0, 0, nullptr, p.ldb64, nullptr};
                const int n_items = (int)cooc_item_count(p.Ic, p.CH, p.nch, false);
                CA.item_seg = F.flat_seg.get() + i_at;
                CA.item_id = F.flat_id.get() + i_at;
                CA.item_grab = cooc_item_grab((size_t)c < P.cluster_deg2.size() ? P.cluster_deg2[c] : P.sum_deg2, n_items);
                fb.push_back(CoocLaunch{CA, ME, n_items, 0});

                const int n_chunks = (int)ceil_div(p.Ic, 64 * VEC);
                // (the chip is filled by all clusters of the batch together: ~8 work-groups per CU over the whole launch)
                const int64_t fill = ceil_div(8 * (int64_t)ctx->num_cus, (int64_t)std::max(1, n_chunks) * (int64_t)n_flat);
                const int n_slices = (int)std::max<int64_t>(1, std::min<int64_t>(tune.max_slices, std::min<int64_t>(ceil_div(nb, 4), std::max<int64_t>(ceil_div(nb, 4 * (int64_t)tune.users_per_wave), fill))));
                FlatDesc d{};
                d.SA = score_args(X, p, Mc, p.ldm, p.a, nb, Sc, p.ldm, n_slices, n_chunks);
                d.n_heavy = F.flat_flags.get() + 2 * k;
                d.any_overflow = F.flat_flags.get() + 2 * k + 1;
                d.SA.n_heavy = tune.score_heavy > 0 ? d.n_heavy : nullptr;
                d.heavy_thresh = tune.score_heavy > 0 ? std::min(tune.score_heavy, 32) : 0x7FFFFFFF;
                d.TA = topn_args(X, p, Sc, p.ldm, p.a);
                d.overflow = F.flat_ov.get() + u_at;
                d.score_grid = n_chunks * n_slices;
                d.n_users = nb;
                const int f = p.pack24 ? 1 : 0;
                max_grid[f] = std::max(max_grid[f], d.score_grid);
                max_users[f] = std::max(max_users[f], nb);
                fd[f].push_back(d);
                m_at += (size_t)round_up((int64_t)p.Ic * p.ldm * (p.pack24 ? 3 : 4), 256);
                s_at += (size_t)nb * p.ldm;
                i_at += (size_t)p.Ic * p.nch;
                u_at += (size_t)nb;
                k++;
            }
            const size_t sp = X.t_cooc->begin(st);
            launch_cooc_rm2_multi(ctx, tune, fb, false, F.d_flat_launch, F.flat_cnt, st, true);
            X.t_cooc->end(sp, st);
            R->st.cooc_launches++;
            for (int f = 0; f < 2; f++) {
                if (fd[f].empty()) continue;
                const unsigned ny = (unsigned)fd[f].size();
                F.d_flat[f].alloc(ctx, fd[f].size());
                FY_HIP(hipMemcpyAsync(F.d_flat[f].get(), fd[f].data(), fd[f].size() * sizeof(FlatDesc), hipMemcpyHostToDevice, st));
                const size_t ss = X.t_score->begin(st);
                k_count_heavy_multi<<<(ny + 63) / 64, 64, 0, st>>>(F.d_flat[f].get(), (int32_t)ny);
                FY_KERNEL_CHECK();
                score_multi_kernel(f != 0, tune.score_walk)<<<dim3((unsigned)max_grid[f], ny), 256, 0, st>>>(F.d_flat[f].get(), P.csr_idx.get(), X.csr_e, X.csr_q, X.pvpi, X.n_out);
                FY_KERNEL_CHECK();
                X.t_score->end(ss, st);
                R->st.score_launches++;
                const size_t tt = X.t_topn->begin(st);
                k_topn_fast_multi<<<dim3((unsigned)max_users[f], ny), 256, 0, st>>>(F.d_flat[f].get(), tune.force_select);
                FY_KERNEL_CHECK();
                k_topn_select_multi<<<dim3((unsigned)max_users[f], ny), 256, 0, st>>>(F.d_flat[f].get(), X.prune_counters + 2);
                FY_KERNEL_CHECK();
                X.t_topn->end(tt, st);
            }
            FY_HIP(hipStreamSynchronize(st));     // the host vectors behind the descriptor uploads leave scope here
        }
        first = last;
    }
}

// ---- 6. two-phase panel mode: every cluster of a group keeps its own panel ...
struct PanelBuf {
    DevBuf<float> Gp, Bmax64, amax64, bmax64;
    DevBuf<uint32_t> Brep;
    DevBuf<double> head32, tail32;     // (refinement pass: per cluster, like the panels -- built in phase 1, read in phase 3)
};
struct PanelPtrs {
    float *Gp, *Bmax64;
    uint32_t* Brep;
    float *amax64, *bmax64;
};
// (host-side sources of uploads and the device buffers of the batched launches: declared in FRONT of the LaneGuard, so that the
// guard -- which drains every lane and the main stream -- is destroyed before them on every path)
struct PanelSet {
    std::vector<PanelBuf> pbuf;        // [plan]
    std::vector<Lane> plane;           // [plan]: the cluster's own scoring scratch
    std::vector<CoocLaunch> batch_main, batch_tail;      // phase 1: the row kernels of all panel clusters, launched together
    DevBuf<CoocLaunch> d_batch_main, d_batch_tail;
    DevBuf<int32_t> d_cnt_main, d_cnt_tail;
    DevBuf<PanelDesc> d_panel_desc;
    std::vector<PanelDesc> hpd;                          // (lives as long as its upload may be in flight)
};
static void group_buffers(Context* ctx, const JobPlan& jp, int seed_chunks, const std::vector<Lane>& lanes, int grp, PanelSet& PS) {
    const std::vector<Plan>& plans = jp.plans;
    std::vector<PanelBuf>& pbuf = PS.pbuf;
    std::vector<Lane>& plane = PS.plane;
    for (size_t pi = 0; pi < plans.size(); pi++) {
        const Plan& p = plans[pi];
        if (!p.panel || jp.group_of[pi] != grp) continue;
        pbuf[pi].Gp.alloc(ctx, (size_t)p.Ic * p.panel_cols * 3 / 4 + 4);
        pbuf[pi].Bmax64.alloc(ctx, (size_t)p.Ic * p.ldb64 * 3 / 4 + 4);
        pbuf[pi].Brep.alloc(ctx, (size_t)p.Ic * p.ldb64 + 4);
        pbuf[pi].amax64.alloc(ctx, (size_t)p.ldb64);
        pbuf[pi].bmax64.alloc(ctx, (size_t)p.ldb64);
    }
    // ... and its own scoring scratch, so that NO host round trip separates the clusters: phase 2 queues seed + bound pass, select, second
    // bound and the survivor count of every cluster, ONE wait reads all counts (pinned host memory), phase 3 queues the survivor
    // passes and top-N.  (With one scratch set per lane the host waited for every cluster's count before it could queue the next
    // cluster of that lane: 50 round trips during which the other lanes ran dry.)
    for (size_t pi = 0; pi < plans.size(); pi++) {
        const Plan& p = plans[pi];
        if (!p.panel || jp.group_of[pi] != grp) continue;
        Lane& W = plane[pi];
        const size_t nbp = (size_t)(p.b - p.a);
        const size_t seed_cols = (size_t)std::min<int64_t>(ceil_div(p.Ic, 256), seed_chunks) * 256;
        W.st = lanes[pi % jp.NS].st;
        W.M.alloc(ctx, 1); W.Bmax.alloc(ctx, 1); W.amax.alloc(ctx, 1); W.bmax.alloc(ctx, 1);
        W.Gp.alloc(ctx, 1); W.Bmax64.alloc(ctx, 1); W.Brep.alloc(ctx, 1); W.amax64.alloc(ctx, 1); W.bmax64.alloc(ctx, 1);
        W.item_seg.alloc(ctx, (size_t)p.Ic * p.nch); W.item_id.alloc(ctx, (size_t)p.Ic * p.nch);
        W.item_seg_t.alloc(ctx, (size_t)std::max(1, p.Ic - p.p_eff)); W.item_id_t.alloc(ctx, (size_t)std::max(1, p.Ic - p.p_eff));
        W.S.alloc(ctx, nbp * seed_cols);
        W.overflow.alloc(ctx, nbp);
        W.any_overflow.alloc(ctx, 1);
        W.n_heavy.alloc(ctx, 1);
        W.UB.alloc(ctx, nbp * (size_t)p.ldb64);
        W.tau.alloc(ctx, nbp);
        W.surv.alloc(ctx, nbp * (size_t)p.ldb64);
        W.surv_mask.alloc(ctx, nbp * (size_t)p.ldb64);
        W.n_quads.alloc(ctx, nbp + 1);
        W.quad_prefix.alloc(ctx, nbp + 1);
    }
}

// Error path: anything thrown while the lanes run (an allocation, a launch, a collective) unwinds the lanes' buffers, the segment
// tables and the per-job arrays back into the caching allocator while kernels of OTHER lanes may still be reading
// them.  The guard drains every lane and the main stream first (objects are destroyed in reverse order of
// declaration: fy_rm2_score declares the lanes, the PanelSet and the per-job arrays before it, so it runs before they are released).
// (The flat batches run on the main stream alone, in front of the guard: their uploads' sources have their own SyncOnUnwind.)
struct LaneGuard {
    Context* ctx;
    hipEvent_t fork = nullptr;
    int32_t* pinned = nullptr;
    ~LaneGuard() {
        for (hipStream_t x : ctx->aux) (void)hipStreamSynchronize(x);
        (void)hipStreamSynchronize(ctx->stream);
        if (fork) (void)hipEventDestroy(fork);
        if (pinned) (void)hipHostFree(pinned);
    }
};

// ---- 7. one cluster on a lane
// one visit of a cluster by the group / phase loop (score_clusters)
struct ClusterVisit {
    size_t pi;                   // its plan
    int grp, phase;
    Lane* L;                     // scratch: the lane's, or (two-phase panel mode, phases 2 and 3) the cluster's own
    hipStream_t ls;
    PanelPtrs PP;
    DevBuf<double>*H32, *T32;    // fp64 head rows / tail columns of the refinement pass: the lane's, or the cluster's own
    Lane* own;                   // two-phase panel mode: the cluster's own scratch (PanelSet::plane), else null
    PanelSet* PS;
    int32_t* pinned;             // two-phase panel mode: [plan] survivor counts, read by the host between phases 2 and 3
};
// What the matrix build and the scoring passes of one cluster share.  The pruned passes write and read only the seed columns and the
// surviving blocks of a score row.
struct ClusterPass {
    const ScoreShared& X;
    const ClusterVisit& V;
    const Plan& p;
    Lane& L;                 // = *V.L, and its stream
    hipStream_t ls;
    Context* ctx;            // X.J's context, structure and the job's knobs
    const Prepared& P;
    const ScoreTune& tune;
    int fxk;                 // exponent of the fixed-point walk, < 0: fp64 accumulators
    double w2s;              // (1-l)^2 (general smoothing: w^2 = 1) and the packed format's 2^-c
    bool refine;             // k_refine_rows: the cluster keeps the unrounded values of its head rows (symmetric panel mode: and of the tail rows' head columns)
    int32_t head_rows;       // ... as many as the seed is wide, 256 .. 1024: N = 50 -> 256, N = 100 -> 512; a multiple of 4
    int64_t ld_head;
    int32_t tail_from;       // first row with a tail32 image (Ic: none)
    int n_chunks;            // 256-column chunks of a score row
    int seed_chunks;         // ... of them scored exactly in front of the bound pass (= the seed blocks)
    bool use_sup;            // bounds over super-blocks, evaluated by the seed chunk's own waves
    const float* Gmat;       // the stored rows: the matrix, or (panel mode) the panel_cols wide panel; gld = their pitch
    int64_t gld, bld, SC;    // bld = pitch of the bound matrix (panel mode: a column per 64-column sub-block), of UB and of the survivor lists;
};                           // SC = pitch of the compact score rows: seed columns only
static ClusterPass cluster_pass(const ScoreShared& X, const ClusterVisit& V) {
    const fy_rm2_job* J = X.J;
    const ScoreTune& tune = *X.tune;
    const Plan& p = X.jp->plans[V.pi];
    ClusterPass C{X, V, p, *V.L, V.ls, J->ctx, J->P, tune};
    C.fxk = (X.jp->use_pk && tune.cooc_fx && !J->fx_bounds.empty()) ? fx_exponent(&J->fx_bounds[3 * (size_t)p.c]) : -1;
    C.w2s = J->S->smooth.w2_of(J->prm.lambda) * (double)X.gscale[(size_t)p.c];
    // (either accumulator the job computes with: the fixed-point sums, or the fp64 sums of the unpacked walk -- a rating of 3.3 must not cost a
    // job its refinement pass; not the fp32 accumulators of the measurement build alone)
    C.refine = tune.refine && p.pack24 && !p.coop && (C.fxk >= 0 || !tune.cooc_f32) && J->S->max_item >= 0 && J->S->max_item < (1 << 28) && p.Ic >= 8;
    C.head_rows = (int32_t)std::min<int64_t>(p.Ic & ~3, std::max<int64_t>(256, std::min<int64_t>(1024, (int64_t)tune.seed_chunks * 256)));
    // the rows that keep their head columns in tail32: symmetric panel mode, the tail rows; the walk from the unpopular side, the rows
    // behind the first chunk (the head rows do not walk them; head rows that all lie in the first chunk store nothing behind it)
    C.tail_from = p.psym ? p.p_eff : p.rect ? p.CH : p.Ic;
    C.ld_head = p.psym ? (int64_t)p.p_eff : (p.rect && C.head_rows <= p.CH) ? (int64_t)p.CH : p.ldm;
    C.n_chunks = (int)ceil_div(p.Ic, 256);
    C.seed_chunks = std::min(C.n_chunks, tune.seed_chunks);
    C.use_sup = tune.sup_bounds && !p.panel && !X.jp->long_seed;
    C.Gmat = p.panel ? V.PP.Gp : V.L->M.get();
    C.gld = p.panel ? (int64_t)p.panel_cols : p.ldm;
    C.bld = p.panel ? p.ldb64 : p.ldb;
    C.SC = (int64_t)C.seed_chunks * 256;
    return C;
}
// FY_DEBUG_SYNC=1: drain the device and say where the job is
static void checkpoint(const ScoreShared& X, const ClusterVisit& V, const char* what) {
    if (X.tune->debug_sync != 1) return;
    const hipError_t e = hipDeviceSynchronize();
    fprintf(stderr, "[fy] group %d/%d phase %d plan %zu (cluster %d): %s -> %s\n", V.grp, X.jp->n_groups, V.phase, V.pi, X.jp->plans[V.pi].c, what, hipGetErrorString(e));
    fflush(stderr);
}

// -- M build: the cluster's matrix (or panel), its block maxima, mirror pass and super-block bounds.  In phase 1 with batched row
// kernels the launches are only collected (PanelSet::batch_main / batch_tail; launch_panel_batch queues them for the whole group).

// one row kernel of the cluster: its item list, then the launch on the lane -- or, batched, its descriptor for the group's launch
// (k_item_list_multi fills the lists in front of it).  `tail`: the tail rows' bound launch.
static void queue_row_kernel(const ScoreShared& X, const ClusterVisit& V, bool batched, bool tail, CoocArgs CA, const MEpilogue& ME, int64_t list_len,
                             int n_items, int item_grab) {
    Lane& L = *V.L;
    int2* const seg = !batched ? L.item_seg.get() : tail ? V.own->item_seg_t.get() : V.own->item_seg.get();
    int32_t* const id = !batched ? L.item_id.get() : tail ? V.own->item_id_t.get() : V.own->item_id.get();
    if (!batched) {
        k_item_list<<<grid_for(list_len), 256, 0, V.ls>>>(CA, seg, id);
        FY_KERNEL_CHECK();
    }
    CA.item_seg = seg; CA.item_id = id; CA.item_grab = item_grab;
    if (batched) {
        (tail ? V.PS->batch_tail : V.PS->batch_main).push_back(CoocLaunch{CA, ME, n_items, 0});
        return;
    }
    FY_HIP(hipMemsetAsync(L.any_overflow.get(), 0, sizeof(int32_t), V.ls));   // reused as the item counter
    launch_cooc_rm2(X.J->ctx, *X.tune, X.jp->use_pk, CA, ME, n_items, L.any_overflow.get(), V.ls);
    X.R->st.cooc_launches++;
}

static void build_cluster_matrix(const ClusterPass& C) {
    const ScoreShared& X = C.X; const ClusterVisit& V = C.V; const Prepared& P = C.P; const ScoreTune& tune = C.tune; const Plan& p = C.p; Lane& L = C.L;
    Context* ctx = C.ctx;
    hipStream_t ls = C.ls;
    const TableCache& tc = X.J->S->tables;
    const JobPlan& jp = *X.jp;
    const PanelPtrs& PP = V.PP;
    const int32_t pbase = p.pbase, Ic = p.Ic;
    const int fxk = C.fxk;
    const double w2s = C.w2s;
    CoocArgs CA = cooc_args(P, tc.segs[V.pi], cooc_geometry(p), X.csr_x, X.csr_pk);
    CA.fx_scale = fxk >= 0 ? std::ldexp(1.0, fxk) : 0.0;
    MEpilogue ME{L.M.get(), p.ldm, (float)w2s, fxk >= 0 ? std::ldexp(w2s, -fxk) : 0.0,
                 p.pack24 ? 1 : 0, (p.prune && !p.panel) ? L.Bmax.get() : nullptr, p.ldb, 0,
                 p.panel ? p.panel_cols : 0, p.panel ? PP.Bmax64 : nullptr, p.ldb64, p.panel ? PP.Brep : nullptr};
    if (p.panel) ME.M = PP.Gp;
    if (C.refine) {
        V.H32->alloc(ctx, (size_t)C.head_rows * C.ld_head + 4);
        if (C.tail_from < Ic) V.T32->alloc(ctx, (size_t)std::max(1, Ic - C.tail_from) * C.head_rows + 4);
        ME.head32 = V.H32->get(); ME.ld_head = C.ld_head; ME.head_rows = C.head_rows;
        ME.tail32 = C.tail_from < Ic ? V.T32->get() : nullptr; ME.tail_from = C.tail_from;
        ME.w2d = w2s;
    }
    if (p.panel) X.R->st.panel_clusters++;
    if (p.panel || p.prune) {     // the bound matrix starts at zero; the maxima of a and b over its blocks (panel mode: 64-column sub-blocks)
        const int64_t bld = p.panel ? p.ldb64 : p.ldb;
        FY_HIP(hipMemsetAsync(p.panel ? PP.Bmax64 : L.Bmax.get(), 0, (size_t)Ic * bld * 3, ls));
        k_block_amax<<<grid_for(bld), 256, 0, ls>>>(Ic, (int32_t)bld, X.a_rank + pbase, X.b_rank + pbase, p.panel ? PP.amax64 : L.amax.get(),
                                                   p.panel ? PP.bmax64 : L.bmax.get(), p.panel ? 64 : PRUNE_BLOCK);
        FY_KERNEL_CHECK();
    }
    const size_t sp = X.t_cooc->begin(ls);
    const bool batched = V.phase == 1 && tune.panel_multi_launch && jp.use_pk && fxk >= 0 && !tune.cooc_f32;     // (k_cooc_rm2_multi)
    if (p.p_eff < Ic) {   // panel mode: bounds of the tail rows behind p_eff (one item per row, see k_tail_blocks)
        CoocGeometry g = cooc_geometry(p);
        g.CH = p.tail_width; g.nch = 1;
        CoocArgs CB = cooc_args(P, tc.segs_tail[V.pi], g, X.csr_x, tc.y_pk.get());
        CB.row0 = p.p_eff; CB.nrows = Ic - p.p_eff; CB.fx_scale = CA.fx_scale;
        MEpilogue MB{reinterpret_cast<float*>(reinterpret_cast<char*>(PP.Bmax64) + (size_t)(p.p_eff / 64) * 3), p.tail_width, ME.w2, ME.fx_inv, 1,
                     nullptr, 0, 0, 0, nullptr, 0, nullptr, p.ldb64, 1};
        queue_row_kernel(X, V, batched, true, CB, MB, Ic - p.p_eff, Ic - p.p_eff, 8);      // (a tail row's bound item is a handful of segments)
        CA.tail_row0 = p.p_eff;
        CA.tail_chunks = p.tail_chunks;
    }
    CA.half = p.rect ? 2 : (p.half || p.psym) ? 1 : 0;
    if (p.psym) { CA.half_rows = p.p_eff; CA.head_chunks = p.tail_chunks; }
    const int n_items = p.psym ? (int)(cooc_half_item_index(p.p_eff - 1, p.tail_chunks - 1, p.CH, p.tail_chunks) + 1 + (int64_t)(Ic - p.p_eff) * p.tail_chunks)
                        : CA.tail_chunks > 0 ? (int)((int64_t)p.p_eff * p.nch + (int64_t)(Ic - p.p_eff) * p.tail_chunks)
                                             : (int)cooc_item_count(Ic, p.CH, p.nch, CA.half);
    const int64_t visits = (size_t)p.c < P.cluster_deg2.size() ? P.cluster_deg2[p.c] : P.sum_deg2;
    queue_row_kernel(X, V, batched, false, CA, ME, (int64_t)Ic * p.nch, n_items, cooc_item_grab(visits / (p.half ? 2 : 1), n_items));
    X.t_cooc->end(sp, ls);
    X.side->join(ls);      // (the scoring kernels behind this point read the per-rating values)
    checkpoint(X, V, "row kernel queued / run");
    if (p.half) {    // lower triangle + the block maxima in front of / on the diagonal
        const size_t sm = X.t_mirror->begin(ls);
        // pruned flow: LAZY mirror -- the seed pass reads the seed columns of every row, the bound pass the block maxima, the
        // survivor pass the surviving column blocks (mirrored below, once they are known); nothing else of the lower triangle
        // is ever read, so it is not written (round 3 moved 10.7 GB here to fill a triangle of which a few per cent were read)
        const bool lazy = p.prune && tune.lazy_mirror;
        launch_mirror(ctx, L.M.get(), p.ldm, Ic, p.prune ? L.Bmax.get() : nullptr, p.ldb, ls, p.rect ? p.CH / 256 : 0, nullptr, lazy ? std::min(tune.seed_chunks, p.nblk) : 0x7FFFFFFF);
        X.t_mirror->end(sm, ls);
    }
    // (not for long lists: their survivors -- 14 % of the blocks at N = 1000 -- spread over the whole popularity order, the 16 wide
    // groups behind the first 48 blocks all survive and hand every block to the survivor pass: measured, the batch falls back to
    // the full pass, 261 -> 471 ms)
    if (p.prune && !p.panel && tune.sup_bounds && !jp.long_seed) {      // super-block bounds for the seed pass (k_score_sup)
        std::vector<int32_t> first;
        sup_block_map(std::min(tune.seed_chunks, p.nblk), p.nblk, first);
        const int n_sup = (int)first.size() - 1;
        first.resize(65, first.back());
        L.sup_first.alloc(ctx, 65);
        L.Bsup.alloc(ctx, (size_t)Ic * 64);
        L.asup.alloc(ctx, 64); L.bsupb.alloc(ctx, 64);
        FY_HIP(hipMemcpyAsync(L.sup_first.get(), first.data(), 65 * sizeof(int32_t), hipMemcpyHostToDevice, ls));
        FY_HIP(hipStreamSynchronize(ls));      // (`first` is a host temporary; one cluster: no other lane is waiting)
        const size_t sb = X.t_score->begin(ls);
        k_build_bsup<<<std::min<int>((Ic + 3) / 4, ctx->num_cus * 32), 256, 0, ls>>>(Ic, n_sup, L.sup_first.get(), L.Bmax.get(), p.ldb, L.Bsup.get());
        FY_KERNEL_CHECK();
        k_sup_amax<<<1, 64, 0, ls>>>(n_sup, L.sup_first.get(), L.amax.get(), L.bmax.get(), L.asup.get(), L.bsupb.get());
        FY_KERNEL_CHECK();
        X.t_score->end(sb, ls);
    }
}

// -- scoring + top-N of the cluster's users of this rank, in user batches that fit the score scratch: the plain full pass, or the
// three pruned passes (seed + bounds, survivor selection, survivors) with the full pass as their fallback.  A two-phase panel
// cluster is visited twice: phase 2 queues the front up to the survivor count, phase 3 the back.

struct UserBatch {           // one batch of the cluster's users
    int32_t s0, nb;
    int n_slices;
    bool whole, split;       // the whole cluster (its CSR range is on the host already); two-phase panel mode: front in phase 2, back in phase 3
};

// scoring arguments of a batch; with FY_SCORE_HEAVY the count of its heavy users is queued in front of the scoring launches
static ScoreArgs batch_score_args(const ClusterPass& C, int32_t s0, int32_t nb, const float* M, int64_t ldm, float* S, int64_t ldS, int n_slices, int n_chunks) {
    ScoreArgs SA = score_args(C.X, C.p, M, ldm, s0, nb, S, ldS, n_slices, n_chunks);
    if (C.tune.score_heavy > 0) {     // (stream order: every scoring launch of the batch follows)
        // a small batch (one cluster of many) cannot fill the chip with a wave per user and its launch lasts as long as its
        // longest list on ONE wave (ML-1M shape in 50 clusters: 0.14 ms per cluster for 120 users): there every user with
        // more than a few batches is walked by a whole workgroup
        const int heavy = (int64_t)nb * n_chunks < 8 * (int64_t)C.ctx->num_cus ? std::min(C.tune.score_heavy, 32) : C.tune.score_heavy;
        k_count_heavy<<<1, 64, 0, C.ls>>>(C.P.rowptr.get() + s0, nb, heavy, C.L.n_heavy.get());
        SA.n_heavy = C.L.n_heavy.get();
    }
    return SA;
}

// ill-conditioned list rows of a range of users, scored again in fp64 from the fp32 head rows (k_refine_rows); after the lists stand
static void refine_rows(const ClusterPass& C, int32_t s0, int32_t nb) {
    if (!C.refine || nb <= 0) return;
    const ScoreShared& X = C.X; const Prepared& P = C.P; const Plan& p = C.p; Lane& L = C.L; hipStream_t ls = C.ls;
    fy_rm2_job* J = X.J;
    const fy_rm2_params& prm = J->prm;
    const size_t tt = X.t_topn->begin(ls);
    const int32_t n_ids = J->S->max_item + 1, head_rows = C.head_rows;
    L.colmap.alloc(C.ctx, (size_t)n_ids);
    FY_HIP(hipMemsetAsync(L.colmap.get(), 0xFF, (size_t)n_ids * sizeof(int32_t), ls));
    k_refine_colmap<<<(head_rows + 255) / 256, 256, 0, ls>>>(head_rows, P.rank_item_raw.get() + p.pbase, L.colmap.get());
    FY_KERNEL_CHECK();
    RefineArgs RA{};
    RA.slot0 = s0; RA.n_users = nb; RA.slot_lo = X.lo; RA.slot_base = p.sbase;
    RA.n_out = X.n_out; RA.out_off = X.out_off; RA.out_item = X.R->d_key1.get(); RA.out_score = X.R->d_value.get(); RA.out_item_w = X.R->d_key1.get();
    RA.rowptr = P.rowptr.get(); RA.csr_idx = P.csr_idx.get(); RA.csr_r = P.csr_r.get(); RA.usum_slot = J->usum_slot.get();
    RA.p_rank = X.p_rank + p.pbase; RA.b_rank = X.b_rank64 + p.pbase;
    RA.colmap = L.colmap.get(); RA.max_item = J->S->max_item; RA.head_rows = head_rows;
    RA.head32 = C.V.H32->get(); RA.ld_head = C.ld_head; RA.tail32 = C.tail_from < p.Ic ? C.V.T32->get() : nullptr; RA.tail_from = C.tail_from;
    RA.rect_ch = p.rect ? p.CH : 0;
    if (!RA.head32 || (C.tail_from < p.Ic && !RA.tail32)) FY_FAIL(FY_ERR_STATE, "internal: cluster %d has no fp32 rows for the refinement pass", p.c);
    RA.unscale = 1.0 / (double)X.gscale[(size_t)p.c];
    RA.general = J->S->smooth.general() ? 1 : 0; RA.G = J->smooth_args(); RA.cluster = p.c;
    RA.lambda = prm.lambda; RA.ln_items = std::log((double)prm.number_of_items); RA.ln_users = std::log((double)p.Uc);
    RA.users_minus_1 = (double)(p.Uc - 1); RA.refine_c = C.tune.refine_c; RA.n_refined = X.prune_counters + 5;
    int lp2 = 64;
    while (lp2 < std::min<int>(prm.number_of_recommendations, p.Ic)) lp2 <<= 1;
    k_refine_rows<<<(nb + 3) / 4, 256, (size_t)4 * lp2 * sizeof(uint64_t), ls>>>(RA);
    FY_KERNEL_CHECK();
    X.t_topn->end(tt, ls);
}

// the lists of a batch from its score rows (TA), then the refinement
static void batch_lists(const ClusterPass& C, int32_t s0, int32_t nb, const TopNArgs& TA, bool long_list) {
    const ScoreShared& X = C.X;
    const size_t tt = X.t_topn->begin(C.ls);
    launch_topn(C.ctx, C.ls, TA, nb, C.L.overflow.get(), C.L.any_overflow.get(), C.tune.force_select, long_list, X.J->prm.number_of_recommendations,
                X.prune_counters + 2);
    X.t_topn->end(tt, C.ls);
    refine_rows(C, s0, nb);
}

// the plain full pass over a range of users: every log term, like the reference's loop (AbstractRM2Reducer.java:332-356)
static void full_pass(const ClusterPass& C, int32_t s0, int32_t nb, float* Sx) {
    const ScoreShared& X = C.X; const Plan& p = C.p;
    const int n_slices = score_slices(C.ctx->num_cus, C.tune, nb, C.n_chunks);
    const ScoreArgs SA = batch_score_args(C, s0, nb, C.L.M.get(), p.ldm, Sx, p.ldm, n_slices, C.n_chunks);
    const size_t ss = X.t_score->begin(C.ls);
    launch_score(score_kernel(p.pack24, C.tune.score_walk), C.n_chunks * n_slices, C.ls, SA);
    X.t_score->end(ss, C.ls);
    X.R->st.score_launches++;
    batch_lists(C, s0, nb, topn_args(X, p, Sx, p.ldm, s0), X.J->prm.number_of_recommendations > TOPN_LONG);
}

// FY_DEBUG_SYNC=3: which blocks survive, and for how many users
static void dump_survivors(const ClusterPass& C, const UserBatch& B) {
    const Plan& p = C.p; Lane& L = C.L;
    DevBuf<int32_t> cnt(C.ctx, (size_t)p.nblk + 1);
    FY_HIP(hipMemsetAsync(cnt.get(), 0, ((size_t)p.nblk + 1) * sizeof(int32_t), C.ls));
    k_surv_block_counts<<<std::min<int>(B.nb, 4096), 64, 0, C.ls>>>(B.nb, L.n_quads.get(), L.surv.get(), p.ldb, cnt.get());
    std::vector<int32_t> hc((size_t)p.nblk + 1);
    FY_HIP(hipMemcpyAsync(hc.data(), cnt.get(), hc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, C.ls));
    FY_HIP(hipStreamSynchronize(C.ls));
    int distinct = 0;
    long long total = 0;
    for (int b2 = 0; b2 < p.nblk; b2++) { distinct += hc[b2] > 0; total += hc[b2]; }
    fprintf(stderr, "[fy] cluster %d: %lld surviving (user, block) pairs in %d distinct blocks of %d:", p.c, total, distinct, p.nblk);
    for (int b2 = 0; b2 < p.nblk; b2++)
        if (hc[b2]) fprintf(stderr, " %d:%d", b2, hc[b2]);
    fprintf(stderr, "\n");
}

// the pruned front: seed + bound launch, tau, block selection, repair, lazy mirror, the scan of the survivor counts
static void pruned_front(const ClusterPass& C, const UserBatch& B) {
    const ScoreShared& X = C.X; const Prepared& P = C.P; const ScoreTune& tune = C.tune; const Plan& p = C.p; Lane& L = C.L; hipStream_t ls = C.ls;
    Context* ctx = C.ctx;
    const PanelPtrs& PP = C.V.PP;
    const int32_t s0 = B.s0, nb = B.nb;
    // (1) + (3) ONE launch: exact scores of the seed columns (the most popular candidates) and the upper bounds of all 256-column
    // blocks (the same kernel on the block-maximum matrix); the grid's tail -- the waves that walk the heaviest users -- is paid once
    // instead of twice.  With super-block bounds the seed chunks' own waves evaluate them and the bound chunks are not launched.
    // (A two-level bound -- 256-column block maxima first, the 64-column sub-block bounds only for the surviving blocks -- was
    // built and measured in round 3: the first level reads a quarter of the bytes, but five times as many blocks reach the
    // second level, whose per-(user, block) gathers of Bmax64 rows cost more than the streamed pass saved: 113 -> 129 ms at 50
    // clusters.  Removed.)
    const int bchunks = (int)(C.bld / 256);
    if (C.use_sup) {
        ScoreArgs SU = batch_score_args(C, s0, nb, C.Gmat, C.gld, L.S.get(), C.SC, B.n_slices, C.seed_chunks);
        L.UBs.alloc(ctx, (size_t)nb * 64);
        SU.Bsup = L.Bsup.get(); SU.asup = L.asup.get(); SU.bsup_b = L.bsupb.get(); SU.UBsup = L.UBs.get();
        SU.n_sup = std::min(64, std::max(0, p.nblk - C.seed_chunks));
        launch_score(score_sup_kernel(tune.score_walk), C.seed_chunks * B.n_slices, ls, SU);
    }
    ScoreArgs SA = batch_score_args(C, s0, nb, C.Gmat, C.gld, L.S.get(), C.SC, B.n_slices, C.seed_chunks + bchunks);
    score_args_bounds(SA, C.seed_chunks, p.panel ? PP.Bmax64 : L.Bmax.get(), C.bld, p.panel ? p.nsub : p.nblk, p.panel ? PP.amax64 : L.amax.get(),
                      p.panel ? PP.bmax64 : L.bmax.get(), L.UB.get());
    if (!C.use_sup) launch_score(score_kernel(true, tune.score_walk), (C.seed_chunks + bchunks) * B.n_slices, ls, SA);
    // (2) tau_u = N-th best seed score; the sorted seed head is also the user's list unless a block survives
    TopNArgs T1 = topn_args(X, p, L.S.get(), C.SC, s0);
    topn_pruned(T1, 1, C.seed_chunks * 256, L.surv.get(), L.n_quads.get(), C.bld, L.tau.get());
    if (X.jp->long_seed) {
        launch_topn_pass(ls, T1, nb, L.overflow.get(), L.any_overflow.get(), 0, true, X.J->prm.number_of_recommendations);
    } else {
        int lp2 = 64;                   // the sort's size: the seed columns, at most TOPN_SAMPLE
        while (lp2 < std::min<int>(std::min<int>(p.Ic, C.seed_chunks * 256), TOPN_SAMPLE)) lp2 <<= 1;
        topn_seed_kernel(lp2, tune.topn_seed_xl)<<<(unsigned)((nb + 3) / 4), 256, 0, ls>>>(T1, nb, L.overflow.get());
        FY_KERNEL_CHECK();
    }
    // (4) the blocks whose bound reaches tau_u, in ascending order
    FY_HIP(hipMemsetAsync(L.n_quads.get(), 0, ((size_t)nb + 1) * sizeof(int32_t), ls));
    if (p.panel)
        k_bound_select_sub<<<grid_for((int64_t)nb * 64, 256), 256, 0, ls>>>(L.UB.get(), C.bld, p.nsub, p.nblk, C.seed_chunks, L.tau.get(),
                                                                           X.pvpi + (s0 - X.lo), nb, C.bld, L.surv.get(), L.surv_mask.get(), L.n_quads.get());
    else if (C.use_sup)
        k_bound_select_sup<<<grid_for((int64_t)nb * 64, 256), 256, 0, ls>>>(L.UBs.get(), std::min(64, std::max(0, p.nblk - C.seed_chunks)), L.sup_first.get(), L.tau.get(),
                                                                           X.pvpi + (s0 - X.lo), nb, p.ldb, L.surv.get(), L.n_quads.get());
    else
        k_bound_select<<<grid_for((int64_t)nb * 64, 256), 256, 0, ls>>>(L.UB.get(), p.ldb, p.nblk, C.seed_chunks, L.tau.get(), X.pvpi + (s0 - X.lo), nb,
                                                                       L.surv.get(), L.n_quads.get());
    FY_KERNEL_CHECK();
    if (tune.debug_sync == 3 && !p.panel) dump_survivors(C, B);
    if (p.panel && tune.panel_repair) {
        // (4b) sub-blocks that hold an item the user rated: bound again without the user's own co-ratings
        RepairArgs RA{L.surv.get(), L.surv_mask.get(), L.n_quads.get(), C.bld, nb, s0, X.lo, p.p_eff, p.Ic, P.rowptr.get(), P.csr_idx.get(),
                      X.csr_x, X.csr_e, X.csr_q, PP.Bmax64, PP.Brep, p.ldb64, PP.amax64, PP.bmax64,
                      L.tau.get(), X.pvpi, (float)C.w2s, X.prune_counters};
        k_bound_repair<<<std::min<int>(nb, ctx->num_cus * 16), 256, 0, ls>>>(RA);
        FY_KERNEL_CHECK();
    }
    if (p.half && !p.panel && tune.lazy_mirror) {      // lazy mirror, second pass: the column blocks with survivors
        const size_t sm = X.t_mirror->begin(ls);
        L.need.alloc(ctx, (size_t)p.nblk + 1);
        FY_HIP(hipMemsetAsync(L.need.get(), 0, ((size_t)p.nblk + 1) * sizeof(int32_t), ls));
        k_flag_surviving_blocks<<<std::min<int>(nb, 4096), 64, 0, ls>>>(nb, L.n_quads.get(), L.surv.get(), p.ldb, L.need.get());
        FY_KERNEL_CHECK();
        launch_mirror(ctx, L.M.get(), p.ldm, p.Ic, nullptr, p.ldb, ls, p.rect ? p.CH / 256 : 0, L.need.get(), 0, false);
        X.t_mirror->end(sm, ls);
    }
    exclusive_scan_i32(ctx, L.n_quads.get(), L.quad_prefix.get(), (size_t)nb + 1, ls, &L.scan_tmp);
}

// The threshold did not bite (e.g. lambda = 0: a user who rated an item nobody else of the cluster rated has only -inf scores,
// tau = -inf keeps every block): the survivor pass would cost more than the plain full pass and 1 KB of scratch per survivor.
// Redo the batch with the full pass, in sub-batches that fit the workspace.
static void fallback_full_pass(const ClusterPass& C, const UserBatch& B) {
    const ScoreShared& X = C.X; const Plan& p = C.p; hipStream_t ls = C.ls;
    if (p.half && C.tune.lazy_mirror) {      // the plain full pass reads every row whole: the rest of the lower triangle now
        const size_t sm = X.t_mirror->begin(ls);
        launch_mirror(C.ctx, C.L.M.get(), p.ldm, p.Ic, nullptr, p.ldb, ls, p.rect ? p.CH / 256 : 0, nullptr, 0x7FFFFFFF, false);
        X.t_mirror->end(sm, ls);
    }
    const int64_t sub = std::max<int64_t>(1, std::min<int64_t>((X.jp->ws / X.jp->NS) / (p.ldm * 4), B.nb));
    DevBuf<float> Sfull(C.ctx, (size_t)(sub * p.ldm));
    for (int32_t t0 = B.s0; t0 < B.s0 + B.nb; t0 += (int32_t)sub) full_pass(C, t0, (int32_t)std::min<int64_t>(sub, B.s0 + B.nb - t0), Sfull.get());
    FY_HIP(hipStreamSynchronize(ls));   // Sfull goes back to the allocator
    X.R->st.prune_fallbacks++;
    X.R->st.score_launches++;          // the fused seed + bound launch that was thrown away
}

// the pruned back: the survivor count reaches the host, then the fallback, or survivors, strays and lists.  `ss` = the open span of
// the scoring timer.
static void pruned_back(const ClusterPass& C, const UserBatch& B, size_t ss) {
    const ScoreShared& X = C.X; const Prepared& P = C.P; const Plan& p = C.p; Lane& L = C.L; hipStream_t ls = C.ls;
    Context* ctx = C.ctx;
    const int32_t s0 = B.s0, nb = B.nb;
    int32_t hv[3] = {0, 0, 0};   // survivors, first / last CSR entry of the batch
    if (!B.split) FY_HIP(hipMemcpyAsync(&hv[0], L.quad_prefix.get() + nb, sizeof(int32_t), hipMemcpyDeviceToHost, ls));
    else hv[0] = C.V.pinned[C.V.pi];
    if (B.whole) {
        hv[1] = (*X.csr_range)[2 * C.V.pi];
        hv[2] = (*X.csr_range)[2 * C.V.pi + 1];
    } else {
        FY_HIP(hipMemcpyAsync(&hv[1], P.rowptr.get() + s0, sizeof(int32_t), hipMemcpyDeviceToHost, ls));
        FY_HIP(hipMemcpyAsync(&hv[2], P.rowptr.get() + s0 + nb, sizeof(int32_t), hipMemcpyDeviceToHost, ls));
    }
    if (!B.split) FY_HIP(hipStreamSynchronize(ls));   // (everything queued on this lane before has finished: Ssurv may be re-sized)
    const int32_t n_surv_total = hv[0];
    const int64_t blocks_checked = (int64_t)nb * std::max(0, p.nblk - C.seed_chunks);
    *X.blocks_total += blocks_checked;
    if (!p.panel && (double)n_surv_total > C.tune.max_surv_frac * (double)blocks_checked) {     // (panel mode has no full matrix to fall back on)
        X.t_score->end(ss, ls);
        fallback_full_pass(C, B);
        *X.fallback_survived += n_surv_total;
        *X.seed_terms_cols += (int64_t)(hv[2] - hv[1]) * (C.seed_chunks * 256 + p.ldb + p.ldm);
        return;
    }
    L.Ssurv.alloc(ctx, (size_t)std::max(1, n_surv_total) * PRUNE_BLOCK);
    if (n_surv_total > 0) {     // (5) exact scores of the survivors, packed: 256 floats per surviving block at entry quad_prefix[u] + k
        const ScoreArgs SQ = batch_score_args(C, s0, nb, C.Gmat, C.gld, L.Ssurv.get(), 0, B.n_slices, C.n_chunks);
        const int panel_blocks = p.panel ? p.panel_cols / 256 : 0x7FFFFFFF;
        score_blocks_kernel(C.tune.score_walk)<<<std::min(n_surv_total, ctx->num_cus * 16), 256, 0, ls>>>(
            SQ.M, SQ.a_rank, P.rowptr.get(), SQ.csr_idx, SQ.csr_e, SQ.csr_q, SQ.pvpi, L.quad_prefix.get(), L.surv.get(), SQ.S, SQ, C.bld, X.prune_counters,
            panel_blocks, p.panel ? L.surv_mask.get() : nullptr);
        FY_KERNEL_CHECK();
        if (p.panel && panel_blocks < p.nblk) {     // survivors behind the panel: exact, from the sparse data
            const size_t slds = ((size_t)p.Uc + 1) * sizeof(int32_t);
            const int sgrid = std::min<int>(n_surv_total, ctx->num_cus * (int)std::max<size_t>(1, std::min<size_t>(6, (150 * 1024) / (slds + 34 * 1024))));
            L.strayT.alloc(ctx, (size_t)sgrid * STRAY_TCAP);
            L.stray_items.alloc(ctx, (size_t)n_surv_total + 1);      // (a group holds at least one surviving block)
            FY_HIP(hipMemsetAsync(L.any_overflow.get(), 0, sizeof(int32_t), ls));   // reused as the item counter
            k_stray_items<<<grid_for(nb), 256, 0, ls>>>(L.quad_prefix.get(), L.surv.get(), C.bld, nb, panel_blocks, L.stray_items.get(),
                                                       L.any_overflow.get());
            FY_KERNEL_CHECK();
            StrayArgs ST{L.quad_prefix.get(), L.surv.get(), L.surv_mask.get(), C.bld, nb, s0, X.lo, p.sbase, p.Uc, panel_blocks, p.Ic, p.pbase,
                         P.rowptr.get(), P.csr_idx.get(), X.csr_e, X.csr_q, P.rank_pair.get(), P.pair_start.get(), P.csc_slot.get(),
                         X.J->S->tables.csc_x.get(), X.a_rank + p.pbase, X.b_rank + p.pbase, X.pvpi,
                         (float)C.w2s, L.Ssurv.get(), L.strayT.get(), X.prune_counters, L.stray_items.get(),
                         L.any_overflow.get()};
            k_score_stray<<<sgrid, 256, slds, ls>>>(ST);
            FY_KERNEL_CHECK();
        }
    }
    X.t_score->end(ss, ls);
    X.R->st.score_launches += 2;   // the fused seed + bound launch and the survivor pass
    // log terms of the seed and bound passes of this batch: (ratings of its users) x (columns walked)
    *X.seed_terms_cols += (int64_t)(hv[2] - hv[1]) * (C.seed_chunks * 256 + (C.use_sup ? 64 : C.bld));
    TopNArgs TA = topn_args(X, p, L.S.get(), C.SC, s0);
    topn_pruned(TA, 2, C.seed_chunks * 256, L.surv.get(), L.n_quads.get(), C.bld, L.tau.get(), L.Ssurv.get(), L.quad_prefix.get());
    batch_lists(C, s0, nb, TA, X.jp->long_seed);
    checkpoint(X, C.V, "back (survivors, strays, lists)");
}

static void score_cluster(const ClusterPass& C) {
    const ScoreShared& X = C.X; const ClusterVisit& V = C.V; const Plan& p = C.p; hipStream_t ls = C.ls;
    for (int32_t s0 = p.a; s0 < p.b; s0 += (int32_t)p.B) {
        const int32_t nb = (int32_t)std::min<int64_t>(p.B, p.b - s0);
        if (!p.prune) { full_pass(C, s0, nb, V.L->S.get()); continue; }
        UserBatch B{s0, nb, score_slices(C.ctx->num_cus, C.tune, nb, C.seed_chunks + (C.use_sup ? 0 : (int)(p.ldb / 256)))};
        B.whole = s0 == p.sbase && nb == p.Uc;
        B.split = X.jp->two_phase && p.panel && B.whole;
        if (V.phase == 3 && !B.split) continue;
        const size_t ss = X.t_score->begin(ls);
        if (V.phase != 3) {
            pruned_front(C, B);
            if (B.split) {      // the count goes to pinned memory; the host does not wait here
                FY_HIP(hipMemcpyAsync(&V.pinned[V.pi], V.L->quad_prefix.get() + nb, sizeof(int32_t), hipMemcpyDeviceToHost, ls));
                X.t_score->end(ss, ls);
                checkpoint(X, V, "front (seed + bound, select, second bound)");
                continue;
            }
        }
        pruned_back(C, B, ss);
    }
}

static void visit_cluster(const ScoreShared& X, const ClusterVisit& V) {
    const JobPlan& jp = *X.jp;
    const Plan& p = jp.plans[V.pi];
    const Lane& L = *V.L;
    const PanelPtrs& PP = V.PP;
    checkpoint(X, V, "start");
    if (p.panel && (!PP.Gp || !PP.Bmax64 || !PP.Brep || !PP.amax64 || !PP.bmax64 || (jp.two_phase && (!L.S.get() || !L.UB.get() || !L.n_quads.get()) && V.phase != 1)))
        FY_FAIL(FY_ERR_STATE, "internal: cluster %d (plan %zu, group %d of %d, phase %d) has no panel buffers", p.c, V.pi, V.grp, jp.n_groups, V.phase);
    if (p.coop) {
        score_cluster_coop(X, p, V.ls);
        return;
    }
    const ClusterPass C = cluster_pass(X, V);
    const bool do_build = !(V.phase >= 2 && p.panel), do_score = V.phase != 1;
    if (do_build) build_cluster_matrix(C);
    if (do_score) score_cluster(C);
}

// phase 1 of a group: the row kernels of all its panel clusters in two launches, then (symmetric panel mode) the lower triangle of
// every panel's square and the head rows' bounds
static void launch_panel_batch(const ScoreShared& X, int grp, PanelSet& PS) {
    Context* ctx = X.J->ctx;
    fy_result* R = X.R;
    const ScoreTune& tune = *X.tune;
    const JobPlan& jp = *X.jp;
    hipStream_t st = ctx->stream;
    std::vector<PanelBuf>& pbuf = PS.pbuf;
    std::vector<CoocLaunch>&batch_main = PS.batch_main, &batch_tail = PS.batch_tail;
    std::vector<PanelDesc>& hpd = PS.hpd;
    DevBuf<PanelDesc>& d_panel_desc = PS.d_panel_desc;
    const size_t sp = X.t_cooc->begin(st);
    launch_cooc_rm2_multi(ctx, tune, batch_tail, true, PS.d_batch_tail, PS.d_cnt_tail, st, true);
    launch_cooc_rm2_multi(ctx, tune, batch_main, false, PS.d_batch_main, PS.d_cnt_main, st, true);
    X.t_cooc->end(sp, st);
    // symmetric panel mode: the lower triangle of every panel's square, then the head rows' bounds (three launches for all clusters)
    int max_cols = 0, max_nsub = 0;
    for (size_t pi = 0; pi < jp.plans.size(); pi++) {
        const Plan& p = jp.plans[pi];
        if (!p.psym || jp.group_of[pi] != grp) continue;
        hpd.push_back(PanelDesc{pbuf[pi].Gp.get(), pbuf[pi].Bmax64.get(), pbuf[pi].Brep.get(), p.panel_cols, p.ldb64, p.Ic, p.p_eff, p.nsub, 0});
        max_cols = std::max(max_cols, p.panel_cols);
        max_nsub = std::max(max_nsub, p.nsub);
    }
    if (!hpd.empty()) {
        // operand check on the host (round 3: these launches faulted at address 0x1000 when a half-built group handed them the
        // descriptors of clusters whose panels were not allocated): every panel pointer set, every shape what the kernels' grids assume
        for (size_t k = 0; k < hpd.size(); k++) {
            const PanelDesc& d = hpd[k];
            if (!d.Gp || !d.Bmax64 || !d.Brep || d.panel_cols <= 0 || d.panel_cols % 256 != 0 || d.p_eff != d.panel_cols || d.Ic < d.p_eff || d.nsub <= 0 ||
                d.ldb64 < d.nsub)
                FY_FAIL(FY_ERR_STATE, "internal: panel %zu of %zu of a batched mirror / column-maximum launch is unusable (Gp %p Bmax64 %p Brep %p panel_cols %d p_eff %d Ic %d nsub %d ldb64 %lld)",
                        k, hpd.size(), (const void*)d.Gp, (const void*)d.Bmax64, (const void*)d.Brep, (int)d.panel_cols, (int)d.p_eff, (int)d.Ic, (int)d.nsub, (long long)d.ldb64);
        }
        const size_t sm = X.t_mirror->begin(st);
        d_panel_desc.alloc(ctx, hpd.size());
        FY_HIP(hipMemcpyAsync(d_panel_desc.get(), hpd.data(), hpd.size() * sizeof(PanelDesc), hipMemcpyHostToDevice, st));
        const unsigned nz = (unsigned)hpd.size();
        if (max_cols / 256 > 1) {
            FY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_mirror_tiles_multi), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * MIRROR_PITCH));
            k_mirror_tiles_multi<<<dim3((unsigned)(max_cols / 128), (unsigned)(max_cols / 256 - 1), nz), 1024, 128 * MIRROR_PITCH, st>>>(d_panel_desc.get());
            FY_KERNEL_CHECK();
        }
        k_mirror_diag_multi<<<dim3((unsigned)(max_cols / 256), nz), 256, 0, st>>>(d_panel_desc.get());
        FY_KERNEL_CHECK();
        k_panel_colmax<<<dim3((unsigned)(max_cols / 256), (unsigned)ceil_div(max_nsub, 16), nz), 256, 0, st>>>(d_panel_desc.get());
        FY_KERNEL_CHECK();
        X.t_mirror->end(sm, st);
    }
    if (tune.debug_sync == 1) {
        const hipError_t e = hipDeviceSynchronize();
        fprintf(stderr, "[fy] group %d/%d: batched row kernels, mirror, column maxima -> %s\n", grp, jp.n_groups, hipGetErrorString(e));
        fflush(stderr);
    }
    R->st.cooc_launches += (batch_tail.empty() ? 0 : 1) + 1;
}

// The clusters outside the flat batches.  One phase (0): every cluster start to end on its lane.  Two-phase panel mode, per group:
// phase 1 = the panels of all panel-mode clusters on the main stream, phase 2 = everything else on the lanes up to the survivor
// counts, phase 3 = the panel clusters' survivor passes and lists.
static void score_clusters(const ScoreShared& X, std::vector<Lane>& lanes, PanelSet& PS, LaneGuard& guard) {
    Context* ctx = X.J->ctx;
    const ScoreTune& tune = *X.tune;
    const JobPlan& jp = *X.jp;
    hipStream_t st = ctx->stream;
    std::vector<PanelBuf>& pbuf = PS.pbuf;
    std::vector<Lane>& plane = PS.plane;
    for (int grp = 0; grp < jp.n_groups; grp++) {
    if (jp.two_phase) {
        if (grp > 0) {       // the previous group's kernels have drained (below): its panels and scratch go back to the allocator
            for (size_t pi = 0; pi < jp.plans.size(); pi++)
                if (jp.plans[pi].panel && jp.group_of[pi] == grp - 1) { pbuf[pi] = PanelBuf(); plane[pi] = Lane(); }
        }
        group_buffers(ctx, jp, tune.seed_chunks, lanes, grp, PS);
        PS.batch_main.clear();
        PS.batch_tail.clear();
        PS.hpd.clear();
    }
    for (int phase = jp.two_phase ? 1 : 0; phase <= (jp.two_phase ? 3 : 0); phase++) {
    const auto host_t0 = std::chrono::steady_clock::now();
    struct PhaseClock {
        const std::chrono::steady_clock::time_point t0;
        int grp, phase;
        bool on;
        ~PhaseClock() {
            if (on) fprintf(stderr, "[fy] group %d phase %d: host queued for %.3f ms\n", grp, phase, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
    } phase_clock{host_t0, grp, phase, tune.debug_sync != 0};
    if (phase == 3) {             // every cluster's survivor count has been queued: one wait for all of them
        for (int l = 0; l < jp.NS; l++) FY_HIP(hipStreamSynchronize(lanes[l].st));
        FY_HIP(hipStreamSynchronize(st));
    }
    if ((phase == 0 || phase == 2) && jp.NS > 1) {   // the lanes start after everything queued on the main stream so far
        if (guard.fork) { FY_HIP(hipEventDestroy(guard.fork)); guard.fork = nullptr; }
        FY_HIP(hipEventCreateWithFlags(&guard.fork, hipEventDisableTiming));
        FY_HIP(hipEventRecord(guard.fork, st));
        for (int l = 0; l < jp.NS; l++) FY_HIP(hipStreamWaitEvent(lanes[l].st, guard.fork, 0));
    }

    for (size_t pi = 0; pi < jp.plans.size(); pi++) {
        const Plan& p = jp.plans[pi];
        if (p.flat) continue;                  // done above
        if (jp.group_of[pi] != grp) continue;     // (clusters outside panel mode are in group 0)
        if ((phase == 1 || phase == 3) && !p.panel) continue;
        const bool own = jp.two_phase && p.panel;      // the cluster's own panel and scratch (PanelSet), else the lane's
        Lane& L = phase == 1 ? lanes[0] : (own ? plane[pi] : lanes[pi % jp.NS]);
        const PanelPtrs PP = own ? PanelPtrs{pbuf[pi].Gp.get(), pbuf[pi].Bmax64.get(), pbuf[pi].Brep.get(), pbuf[pi].amax64.get(), pbuf[pi].bmax64.get()}
                                 : PanelPtrs{L.Gp.get(), L.Bmax64.get(), L.Brep.get(), L.amax64.get(), L.bmax64.get()};
        visit_cluster(X, ClusterVisit{pi, grp, phase, &L, phase == 1 ? st : L.st, PP, own ? &pbuf[pi].head32 : &L.head32, own ? &pbuf[pi].tail32 : &L.tail32,
                                      own ? &plane[pi] : nullptr, &PS, guard.pinned});
    }
    if (phase == 1 && (!PS.batch_main.empty() || !PS.batch_tail.empty())) launch_panel_batch(X, grp, PS);
    if (tune.debug_sync == 2) {
        (void)hipDeviceSynchronize();
        fprintf(stderr, "[fy] group %d phase %d: %.3f ms from its first queued operation to the drained device\n", grp, phase,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count());
    }
    }      // phase
    if (grp + 1 < jp.n_groups) {     // the next group re-uses this group's memory: everything queued so far must have finished
        for (int l = 0; l < jp.NS; l++) FY_HIP(hipStreamSynchronize(lanes[l].st));
        FY_HIP(hipStreamSynchronize(st));
    }
    }      // group
    if (jp.NS > 1) {   // join: the main stream continues after every lane has drained
        for (int l = 0; l < jp.NS; l++) {
            hipEvent_t done;
            FY_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
            FY_HIP(hipEventRecord(done, lanes[l].st));
            FY_HIP(hipStreamWaitEvent(st, done, 0));
            FY_HIP(hipEventDestroy(done));
        }
    }
}

// ---- 8. what the job says about itself: counters of the pruned passes, the tables, the bytes the row kernels stored
static void fill_score_stats(const ScoreShared& X, const std::vector<int32_t>& sig) {
    fy_rm2_job* J = X.J;
    Context* ctx = X.J->ctx;
    fy_result* R = X.R;
    const JobPlan& jp = *X.jp;
    TableCache& tc = J->S->tables;
    unsigned long long hc[6];
    d2h(ctx, hc, X.prune_counters, 6);
    sync(ctx);
    tc.sig = sig;          // every table of the plan has been built and used: a later job with the same plan re-uses them
    tc.valid = true;
    R->st.cooc_segments = tc.store.n_seg;
    for (auto& p : jp.plans) {       // what the row kernels store (the mirror pass and the column maxima are priced separately)
        const int64_t eb = p.pack24 ? 3 : 4;
        if (p.coop) continue;
        if (p.panel) R->st.cooc_matrix_bytes += (int64_t)p.Ic * p.panel_cols * 3 + (int64_t)p.Ic * p.ldb64 * 7;
        else R->st.cooc_matrix_bytes += eb * (p.half ? (int64_t)p.Ic * (p.Ic + 256) / 2 : (int64_t)p.Ic * p.Ic) + (p.prune ? (int64_t)p.Ic * p.nblk * 3 : 0);
    }
    R->st.topn_select_users = (int64_t)hc[2];
    R->st.stray_blocks = (int64_t)hc[3];
    R->st.bound_repairs = (int64_t)hc[4];
    R->st.rows_refined = (int64_t)hc[5];
    R->st.blocks_survived = (int64_t)hc[0] + *X.coop_survived + *X.fallback_survived;
    R->st.blocks_total = *X.blocks_total;
    R->st.log_terms_evaluated = *X.blocks_total ? (int64_t)hc[1] + *X.seed_terms_cols : 0;
}

// what plan_job reads of the job (the owner ranges and n_recs are filled in by fy_rm2_score once they are known)
static PlanInput plan_input(const fy_rm2_job* J) {
    const Prepared& P = J->P;
    const fy_rm2_params& prm = J->prm;
    PlanInput in;
    in.K = P.K;
    in.nU = P.nU;
    in.csize = P.csize;
    in.ucstart = P.ucstart;
    in.pcstart = P.pcstart;
    in.cluster_q = P.cluster_q;
    in.cluster_deg2 = P.cluster_deg2;
    in.sum_deg2 = P.sum_deg2;
    in.ratings_fp16_exact = P.ratings_fp16_exact;
    in.fx_bounds = J->fx_bounds;
    in.number_of_recommendations = prm.number_of_recommendations;
    in.rank = prm.rank;
    in.world = prm.world;
    in.lambda = prm.lambda;
    in.general_smoothing = J->S->smooth.general();
    in.workspace_bytes = prm.workspace_bytes;
    in.tune = J->ctx->tune;
    in.total_mem = J->ctx->total_mem;
    in.sharded = J->S->sharded;
    in.have_coll = J->have_coll;
    return in;
}
static void fill_request_view(fy_rm2_job* J, RequestView& V);

// ---- the RM1 estimator (FY_RM2_ESTIMATOR_RM1): the side outputs of every job, then one fp64 pass over the rank's slots (fy_rm1.hip)
static void score_rm1(fy_rm2_job* J, fy_result* R) {
    Context* ctx = J->ctx;
    const Prepared& P = J->P;
    hipStream_t st = ctx->stream;
    DevBuf<double> icoll_mine, d_total(ctx, 1);
    if (J->S->sharded) icoll_mine.alloc(ctx, P.nI); else R->d_icoll.alloc(ctx, P.nI);
    k_item_coll<<<grid_for(P.nI), 256, 0, st>>>(P.nI, J->stats.get(), J->S->sharded ? icoll_mine.get() : R->d_icoll.get(), d_total.get());
    FY_KERNEL_CHECK();
    for (int c = 0; c < P.K; c++)
        if (P.csize[c] > 0) R->st.n_clusters_nonempty++;
    RequestView V;
    fill_request_view(J, V);
    std::vector<int32_t> slots((size_t)std::max(0, J->slot_hi - J->slot_lo));
    for (size_t k = 0; k < slots.size(); k++) slots[k] = J->slot_lo + (int32_t)k;
    rm1_score_slots(V, slots, R);
    R->rq = fy_rm2_request_stats{};      // (a full job's result carries no request statistics)
    if (J->S->sharded) {
        sharded_side_outputs(J, R, d_total.get());
    } else {
        R->d_user_id.alloc(ctx, P.nU);
        R->d_user_sum.alloc(ctx, P.nU);
        d2d(ctx, R->d_user_id.get(), P.uid.get(), P.nU);
        d2d(ctx, R->d_user_sum.get(), P.usum.get(), P.nU);
        R->d_item_id.alloc(ctx, P.nI);
        d2d(ctx, R->d_item_id.get(), P.iid.get(), P.nI);
    }
    d2h(ctx, &R->total_sum, d_total.get(), 1);
    sync(ctx);
}

fy_result* fy::rm2_score(fy_rm2_job* J) {
    Context* ctx = J->ctx;
    Prepared& P = J->P;
    const fy_rm2_params& prm = J->prm;
    hipStream_t st = ctx->stream;
    if (!J->have_global) {
        if (prm.world == 1) rm2_set_global_stats(J, J->partial.get(), 1);
        else if (J->have_coll) {   // the all-gather of the per-item statistics (jobs RM2-1 / RM2-2) through the installed collectives
            const int64_t len = J->S->exchange_len();
            J->gathered.alloc(ctx, (size_t)(len * prm.world));
            coll_all_gather(J, J->S->sharded ? J->S->partial_raw.get() : J->partial.get(), J->gathered.get(), len * (int64_t)sizeof(double), st);
            rm2_set_global_stats(J, J->gathered.get(), prm.world);
        } else
            FY_FAIL(FY_ERR_STATE, "world > 1: call fy_rm2_set_global_stats (or install fy_collectives) before fy_rm2_score");
    }
    std::unique_ptr<fy_result> R(new fy_result);
    R->ctx = ctx;
    R->kind = 0;
    R->st.nnz = P.nnz;
    R->st.n_users = P.nU;
    R->st.n_items = P.nI;
    R->st.ms_prepare = J->ms_prepare;
    R->st.prepared_from_cache = J->from_cache ? 1 : 0;
    EventTimer t_total(ctx), t_cooc(ctx), t_score(ctx), t_topn(ctx), t_tables(ctx), t_mirror(ctx);
    const size_t span_total = t_total.begin();
    size_t span_tables = t_tables.begin();
    if (P.nnz == 0) {
        if (J->S->sharded) {      // nothing to score here, but the side outputs are everybody's
            DevBuf<double> d_total(ctx, 1);
            k_item_coll<<<1, 64, 0, st>>>(0, J->stats.get(), nullptr, d_total.get());
            FY_KERNEL_CHECK();
            sharded_side_outputs(J, R.get(), d_total.get());
            d2h(ctx, &R->total_sum, d_total.get(), 1);
            sync(ctx);
        }
        t_total.end(span_total);
        sync(ctx);
        return R.release();
    }
    const int32_t nU = P.nU, nI = P.nI;
    PlanInput in = plan_input(J);
    const bool rm1 = (prm.flags & FY_RM2_ESTIMATOR_RM1) != 0;
    if (J->S->smooth.general() || rm1) {
        // The cooperative path (fy_rm2_coop.hpp) knows RM2 with Jelinek-Mercer alone.  Whether a cluster would take it is host arithmetic: the
        // plan is made once ahead with a stand-in for the number of list rows, and such a job is refused before anything is queued.
        PlanInput dry = in;
        J->count_balanced = plan_count_balanced(dry);
        dry.own_lo.resize((size_t)prm.world);
        dry.own_hi.resize((size_t)prm.world);
        for (int k = 0; k < prm.world; k++) owner_range(J, k, dry.own_lo[(size_t)k], dry.own_hi[(size_t)k]);
        dry.n_recs = 1;
        bool would_coop = false;
        try {
            would_coop = plan_job(dry).any_coop;
        } catch (const PlanError&) {      // (the job's own plan below reports it)
        }
        if (would_coop && rm1)
            FY_FAIL(FY_ERR_UNSUPPORTED, "fy_rm2_score: a cluster of this job would be scored cooperatively by all ranks, which supports the RM2 estimator "
                                        "only (FY_RM2_ESTIMATOR_RM1: run without collectives)");
        if (would_coop)
            FY_FAIL(FY_ERR_UNSUPPORTED, "fy_rm2_score: a cluster of this job would be scored cooperatively by all ranks, which supports Jelinek-Mercer "
                                        "smoothing only (FY_RM2_SMOOTHING_DIRICHLET / FY_RM2_SMOOTHING_ABSOLUTE_DISCOUNT: run without collectives)");
    }
    if (rm1) {
        score_rm1(J, R.get());
        t_total.end(span_total);
        sync(ctx);
        R->st.ms_total = t_total.total_ms();
        return R.release();
    }
    ScoreTune tune = ctx->tune;
    tune.seed_chunks = plan_seed(tune, prm.number_of_recommendations).seed_chunks;     // (0 = from the list length)
    const bool use_pk = tune.cooc_pk && P.ratings_fp16_exact;   // packed CSR for the row kernel
    const PackPlan pack = plan_pack24(in);

    // ---- 1. the preamble
    JobArrays A;
    SideValues side(ctx);
    score_preamble(J, R.get(), pack, use_pk, A, side);
    t_tables.end(span_tables);

    // ---- 2. which users this rank emits lists for; their meta and output offsets
    J->count_balanced = plan_count_balanced(in);
    in.own_lo.resize((size_t)prm.world);
    in.own_hi.resize((size_t)prm.world);
    for (int k = 0; k < prm.world; k++) owner_range(J, k, in.own_lo[(size_t)k], in.own_hi[(size_t)k]);
    const int32_t lo = in.own_lo[(size_t)prm.rank], hi = in.own_hi[(size_t)prm.rank];
    UserMeta U;
    in.n_recs = user_meta_and_offsets(J, R.get(), lo, hi, A.d_cshift.get(), U);
    for (int c = 0; c < P.K; c++)
        if (P.csize[c] > 0) R->st.n_clusters_nonempty++;

    // ---- the plan (pure host arithmetic: fy_rm2_plan.hpp)
    JobPlan jp;
    try {
        jp = plan_job(in);
    } catch (const PlanError& e) {
        FY_FAIL(e.code, "%s", e.msg.c_str());
    }
    int64_t coop_pair_contribs = 0;
    if (in.n_recs > 0 && jp.max_Ic > 0) {
        const std::vector<Plan>& plans = jp.plans;
        cooc_rm2_allow_lds(tune.cooc_epi);
        stray_allow_lds();
        // (the side stream's per-rating values, see SideValues: only the plain one-cluster flow lets them run beside its row kernel)
        if (!(jp.NS == 1 && plans.size() == 1 && !plans[0].coop && !plans[0].flat && !plans[0].panel)) side.join(st);

        // ---- 3. lanes
        std::vector<Lane> lanes((size_t)jp.NS);
        alloc_lanes(ctx, jp, lanes);
        DevBuf<unsigned long long> prune_counters(ctx, 6);   // (ScoreShared::prune_counters)
        prune_counters.zero();
        int64_t prune_blocks_total = 0, prune_seed_terms_cols = 0, coop_survived = 0, fallback_survived = 0;

        // ---- 4. tables
        TableCache& tc = J->S->tables;
        const std::vector<int32_t> sig = table_signature(jp);
        const bool tables_cached = tc.valid && tc.sig == sig;
        R->st.tables_from_cache = tables_cached ? 1 : 0;
        span_tables = t_tables.begin();
        std::vector<int32_t> csr_range;
        build_job_tables(J, jp, tables_cached, csr_range);
        t_tables.end(span_tables);

        const ScoreShared X{J, R.get(), &tune, &jp, A.b_rank32.get(), J->b_rank.get(), A.p_rank.get(), A.a_rank.get(),
                            use_pk ? tc.csc_x_over_s.get() : tc.csc_x.get(), A.csr_x.get(), A.csr_e.get(), A.csr_q.get(), use_pk ? tc.csr_pk.get() : nullptr,
                            U.n_out.get(), U.out_off.get(), U.pvpi.get(), lo, &csr_range, &side, &t_cooc, &t_score, &t_topn, &t_mirror, prune_counters.get(),
                            &prune_blocks_total, &prune_seed_terms_cols, &coop_survived, &fallback_survived, &coop_pair_contribs, A.d_cshift.get(),
                            jp.h_gscale.data()};

        // ---- 5. flat batches
        FlatBuffers flat;
        score_flat_batches(X, flat);

        // ---- 6. + 7. every other cluster on its lane (two-phase panel mode: group by group)
        PanelSet PS;
        PS.pbuf.resize(jp.two_phase ? plans.size() : 0);
        PS.plane.resize(jp.two_phase ? plans.size() : 0);
        LaneGuard guard{ctx};
        if (jp.two_phase) FY_HIP(hipHostMalloc(reinterpret_cast<void**>(&guard.pinned), plans.size() * sizeof(int32_t), hipHostMallocDefault));
        score_clusters(X, lanes, PS, guard);
        // (the guard's destructor drains the lanes and the main stream before any buffer of this scope is released)

        // ---- 8. stats
        fill_score_stats(X, sig);
    }
    // rm2/userSum and rm2/itemColl stay in HBM until somebody asks for them
    if (J->S->sharded) {
        sharded_side_outputs(J, R.get(), A.d_total.get());
    } else {
        R->d_user_id.alloc(ctx, nU);
        R->d_user_sum.alloc(ctx, nU);
        d2d(ctx, R->d_user_id.get(), P.uid.get(), nU);
        d2d(ctx, R->d_user_sum.get(), P.usum.get(), nU);
        R->d_item_id.alloc(ctx, nI);
        d2d(ctx, R->d_item_id.get(), P.iid.get(), nI);
    }
    t_total.end(span_total);
    d2h(ctx, &R->total_sum, A.d_total.get(), 1);
    sync(ctx);
    // (bench.py prices the row kernel with (pair_contribs - nnz) / 2 unordered pairs: a cooperative rank walked only its rows)
    R->st.pair_contribs = jp.any_coop ? coop_pair_contribs + P.nnz : P.sum_deg2;
    R->st.ms_cooc = t_cooc.total_ms();
    R->st.ms_score = t_score.total_ms();
    R->st.ms_topn = t_topn.total_ms();
    R->st.ms_total = t_total.total_ms();
    R->st.ms_tables = t_tables.total_ms();
    R->st.ms_mirror = t_mirror.total_ms();
    return R.release();
}

void fy::rm2_set_collectives(fy_rm2_job* J, const fy_collectives* c) {
    if (!c || !c->all_gather || !c->reduce_scatter_f32) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "fy_collectives needs all_gather and reduce_scatter_f32");
    J->coll = *c;
    J->have_coll = true;
}

// what a restricted request (fy_rm2_request.hip) reads of the job
void fy::rm2_request_view(fy_rm2_job* J, RequestView& V) {
    if (J->have_coll) FY_FAIL(FY_ERR_UNSUPPORTED, "fy_rm2_score_users: the job has collectives installed (the cooperative path serves no requests)");
    if (!J->have_global) {
        if (J->prm.world == 1) rm2_set_global_stats(J, J->partial.get(), 1);
        else FY_FAIL(FY_ERR_STATE, "world > 1: call fy_rm2_set_global_stats before fy_rm2_score_users");
    }
    fill_request_view(J, V);
}

void fy::rm2_job_peek(const fy_rm2_job* J, fy_rm2_params* prm, bool* have_coll) {
    *prm = J->prm;
    *have_coll = J->have_coll;
}

static void fill_request_view(fy_rm2_job* J, RequestView& V) {
    V.ctx = J->ctx;
    V.prm = J->prm;
    V.P = &J->P;
    V.slot_lo = J->slot_lo;
    V.slot_hi = J->slot_hi;
    V.have_coll = J->have_coll;
    V.stats = J->stats.get();
    V.b_rank = J->b_rank.get();
    V.walk_rank = J->walk_rank.get();
    V.usum_slot = J->usum_slot.get();
    V.general = J->S->smooth.general();
    if (V.general) { V.G = J->smooth_args(); V.fx_rank = J->fx_rank.get(); V.fx_bounds = J->fx_bounds.data(); }
    V.state = &J->S->request_state;
}

void fy::rm2_partial_stats(fy_rm2_job* J, double** buf, int64_t* len) {
    *buf = J->S->sharded ? J->S->partial_raw.get() : J->partial.get();
    *len = J->S->exchange_len();
}

void fy::rm2_stats_layout(fy_rm2_job* J, int64_t* n_item_slots, int64_t* n_user_slots) {
    *n_item_slots = J->S->sharded ? J->S->n_raw_items : (int64_t)J->P.nI;
    *n_user_slots = J->S->sharded ? J->S->n_raw_users : 0;
}

void fy::rm2_job_destroy(fy_rm2_job* J) {
    if (!J) return;
    Context* ctx = J->ctx;
    // nothing of the job may still be read by a queued kernel when its arrays go back to the caching allocator
    for (hipStream_t x : ctx->aux) (void)hipStreamSynchronize(x);
    (void)hipStreamSynchronize(ctx->stream);
    delete J;
}
