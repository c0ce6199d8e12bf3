// fy_eval.hip -- offline evaluation on the GPU (include/filmyou.h, "offline evaluation").
//
//   holdout  : one streaming pass over the COO in the shape of fy_ratings_update.hip's source pass: every wave owns a contiguous range,
//              counts its test entries (ballot + popcount), an inclusive scan over the waves' counts gives every wave its place, the
//              second pass writes both sides in source order: a test entry goes to (test entries before it), a train entry to
//              (its position - test entries before it).  The decision is a hash of the key alone.
//   lists    : rows from elsewhere become a list result; the list heads' users are sorted and a repeated user is refused.
//   prepare  : (user << 32 | item) keys of the test ratings, radix-sorted; duplicates flagged; the relevant entries compacted into one
//              ascending item row per user; a table of the distinct users with row starts; for graded gains a second sort by
//              (user, descending score) from which one wave per user sums IDCG at every cutoff in a fixed order.
//   evaluate : list heads from the user column + a scan; ONE WAVE PER LIST walks its list in chunks of 64 positions, lane l
//              binary-searches its item in the user's relevant row, the chunk's hit mask is one ballot: cumulative hits at a lane are
//              the carry plus the popcount of the mask up to the lane, the first hit is a find-first-set, hits_N a popcount of the
//              clipped mask.  Per-lane fp64 partials of AP and DCG per cutoff meet in a fixed xor butterfly.  The per-list values
//              go to HBM; a second kernel adds them over fixed slices in a fixed order, a third adds the slices: the sums are the
//              same bits on every run.
#include <cmath>

#include "fy_eval.hpp"
#include "fy_prep.hpp"
#include "fy_rm2.hpp"

namespace fy {

namespace {

inline int small_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, 256), 4096)); }

__device__ __forceinline__ uint64_t ev_key(int32_t u, int32_t i) { return ((uint64_t)(uint32_t)u << 32) | (uint32_t)i; }

// ---------------------------------------------------------------- hold-out split
constexpr int HO_BLOCK = 256;
constexpr int HO_WAVES = HO_BLOCK / 64;

struct Holdout {
    int64_t nnz, per;               // entries, entries per wave (a multiple of 64)
    const int32_t* user;
    const int32_t* item;
    const float* score;
    uint64_t seed_term;             // seed * 0x9E3779B97F4A7C15
    uint64_t threshold;             // floor(fraction * 2^24)
};

__device__ __forceinline__ bool ho_is_test(int32_t u, int32_t i, uint64_t seed_term, uint64_t threshold) {
    uint64_t z = ev_key(u, i) + seed_term;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (z >> 40) < threshold;
}

// WRITE = false: wave_count[w] = test entries of wave w's range.
// WRITE = true : both sides in source order; wave w's first test entry goes to wave_incl[w - 1].
template <bool WRITE>
__global__ void __launch_bounds__(HO_BLOCK) k_holdout(Holdout S, int64_t* __restrict__ wave_count, const int64_t* __restrict__ wave_incl,
                                                      int32_t* __restrict__ tr_user, int32_t* __restrict__ tr_item, float* __restrict__ tr_score,
                                                      int32_t* __restrict__ te_user, int32_t* __restrict__ te_item, float* __restrict__ te_score) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * HO_WAVES + (threadIdx.x >> 6);
    const int64_t lo = w * S.per < S.nnz ? w * S.per : S.nnz, hi = lo + S.per < S.nnz ? lo + S.per : S.nnz;
    int64_t off = 0;                                            // test entries in front of the current chunk
    if (WRITE) off = w ? wave_incl[w - 1] : 0;
    for (int64_t base = lo; base < hi; base += 64) {            // wave-uniform trip count: every lane enters every ballot
        const int64_t t = base + lane;
        const bool in = t < hi;
        const int32_t u = in ? S.user[t] : 0, i = in ? S.item[t] : 0;
        const bool to_test = in && ho_is_test(u, i, S.seed_term, S.threshold);
        const unsigned long long mask = __ballot(to_test);
        if (WRITE && in) {
            const int64_t before = off + __popcll(mask & ((1ull << lane) - 1ull));
            const float s = S.score[t];
            if (to_test) {
                te_user[before] = u; te_item[before] = i; te_score[before] = s;
            } else {
                tr_user[t - before] = u; tr_item[t - before] = i; tr_score[t - before] = s;
            }
        }
        off += __popcll(mask);
    }
    if (!WRITE && lane == 0) wave_count[w] = off;
}

// ---------------------------------------------------------------- list heads (a row is a head iff it is row 0 or its user differs from the row before)
__global__ void k_ev_heads(int32_t n, const int32_t* __restrict__ key0, uint32_t* __restrict__ head) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) head[t] = t == 0 || key0[t] != key0[t - 1];
}
// lstart[l] = first row of list l, lstart[n_lists] = n; luser_key (may be NULL): the head's user as a sort key
__global__ void k_ev_list_starts(int32_t n, const int32_t* __restrict__ key0, const uint32_t* __restrict__ head, const uint32_t* __restrict__ head_incl,
                                 int32_t* __restrict__ lstart, uint64_t* __restrict__ luser_key) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        if (head[t]) {
            lstart[head_incl[t] - 1] = t;
            if (luser_key) luser_key[head_incl[t] - 1] = (uint32_t)key0[t];
        }
        if (t == n - 1) lstart[head_incl[t]] = n;
    }
}
__global__ void k_ev_adjacent_equal(int32_t n, const uint64_t* __restrict__ sorted, uint32_t* __restrict__ flag) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t + 1 < n; t += gridDim.x * blockDim.x)
        if (sorted[t] == sorted[t + 1]) flag[0] = 1u;           // every writer stores the same word
}

// ---------------------------------------------------------------- prepare
__global__ void k_ev_pack(int32_t n, const int32_t* __restrict__ user, const int32_t* __restrict__ item, uint64_t* __restrict__ keys, uint32_t* __restrict__ pos) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        keys[t] = ev_key(user[t], item[t]);
        pos[t] = (uint32_t)t;
    }
}
// rel[t]: sorted entry t is relevant ((double) score >= threshold; NaN compares false); flag[0] = 1 when two entries share a key
__global__ void k_ev_relevant(int32_t n, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ spos, const float* __restrict__ score, double threshold,
                              uint32_t* __restrict__ rel, uint32_t* __restrict__ flag) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        rel[t] = (double)score[spos[t]] >= threshold;
        if (t + 1 < n && skeys[t] == skeys[t + 1]) flag[0] = 1u;
    }
}
__device__ __forceinline__ double ev_gain(int kind, float score) {
    return kind == FY_EVAL_GAIN_LINEAR ? (double)score : kind == FY_EVAL_GAIN_EXP2 ? exp2((double)score) - 1.0 : 1.0;
}
// the relevant entries, still ascending by (user, item); graded gains: the gain and the key of the second sort, (user, ~bits(score)):
// a relevant score is positive there (threshold > 0), and a positive float's bit pattern is monotone, as is the gain in the score
__global__ void k_ev_compact(int32_t n, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ spos, const float* __restrict__ score,
                             const uint32_t* __restrict__ rel, const uint32_t* __restrict__ rel_incl, int gain_kind, uint64_t* __restrict__ ckey,
                             double* __restrict__ cgain, uint64_t* __restrict__ gkey, uint32_t* __restrict__ gpos) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x)
        if (rel[t]) {
            const uint32_t j = rel_incl[t] - 1;
            ckey[j] = skeys[t];
            if (gain_kind != FY_EVAL_GAIN_BINARY) {
                const float s = score[spos[t]];
                cgain[j] = ev_gain(gain_kind, s);
                gkey[j] = (skeys[t] & 0xFFFFFFFF00000000ull) | (uint32_t)~__float_as_uint(s);
                gpos[j] = j;
            }
        }
}
__global__ void k_ev_user_heads(int32_t m, const uint64_t* __restrict__ ckey, uint32_t* __restrict__ head) {
    for (int32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x)
        head[j] = j == 0 || (ckey[j] >> 32) != (ckey[j - 1] >> 32);
}
__global__ void k_ev_table(int32_t m, const uint64_t* __restrict__ ckey, const uint32_t* __restrict__ head, const uint32_t* __restrict__ head_incl,
                           uint32_t* __restrict__ tuser, int32_t* __restrict__ tstart, uint32_t* __restrict__ titem) {
    for (int32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        titem[j] = (uint32_t)ckey[j];
        if (head[j]) {
            tuser[head_incl[j] - 1] = (uint32_t)(ckey[j] >> 32);
            tstart[head_incl[j] - 1] = j;
        }
        if (j == m - 1) tstart[head_incl[j]] = m;
    }
}
__global__ void k_ev_gather_gain(int32_t m, const double* __restrict__ cgain, const uint32_t* __restrict__ order, double* __restrict__ sorted) {
    for (int32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) sorted[j] = cgain[order[j]];
}

struct Cutoffs {
    int32_t n, last;
    int32_t at[FY_EVAL_MAX_CUTOFFS];
};

// the fixed butterfly every per-wave fp64 sum of this file ends in
__device__ __forceinline__ double ev_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per user: IDCG at every cutoff.  Binary gain: a prefix of the discount table (cum[k] = the first k discounts added in
// order); graded: the user's gains in descending order times the discounts, lane l takes positions l, l + 64, ...
__global__ void __launch_bounds__(256) k_ev_idcg(int32_t n_users, const int32_t* __restrict__ tstart, const double* __restrict__ sorted_gain,
                                                 const double* __restrict__ discount, const double* __restrict__ cum, Cutoffs C,
                                                 double* __restrict__ idcg) {
    const int lane = threadIdx.x & 63;
    const int32_t k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_users) return;
    const int32_t s = tstart[k], cnt = tstart[k + 1] - s;
    if (!sorted_gain) {
        if (lane < C.n) idcg[(int64_t)k * C.n + lane] = cum[min(cnt, C.at[lane])];
        return;
    }
    double part[FY_EVAL_MAX_CUTOFFS];
#pragma unroll
    for (int c = 0; c < FY_EVAL_MAX_CUTOFFS; c++) part[c] = 0.0;
    const int32_t lim = min(cnt, C.last);
    for (int32_t p0 = lane; p0 < lim; p0 += 64) {
        const double g = sorted_gain[s + p0] * discount[p0];
#pragma unroll
        for (int c = 0; c < FY_EVAL_MAX_CUTOFFS; c++)
            if (c < C.n && p0 < C.at[c]) part[c] += g;
    }
#pragma unroll
    for (int c = 0; c < FY_EVAL_MAX_CUTOFFS; c++) {
        const double v = ev_wave_sum(part[c]);
        if (lane == 0 && c < C.n) idcg[(int64_t)k * C.n + c] = v;
    }
}

// ---------------------------------------------------------------- the metric kernel
struct EvalLists {
    int32_t n_lists;
    const int32_t* lstart;          // n_lists + 1
    const int32_t* key0;            // user of every row
    const int32_t* key1;            // item of every row
    int32_t n_users;
    const uint32_t* tuser;          // the evaluator's tables
    const int32_t* tstart;
    const uint32_t* titem;
    const double* tgain;            // NULL: binary
    const double* idcg;
    const double* discount;
    Cutoffs C;
};

constexpr int EV_VALUES = 5;        // hits, recall, AP, RR, nDCG per cutoff

// out[l][c][0..4]; NaN for a list whose user has no relevant entry
__global__ void __launch_bounds__(256) k_ev_metrics(EvalLists E, double* __restrict__ out) {
    extern __shared__ double ev_disc[];                         // C.last discounts (at most 32 KiB), staged once per block
    for (int k = threadIdx.x; k < E.C.last; k += 256) ev_disc[k] = E.discount[k];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int32_t l = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (l >= E.n_lists) return;
    const int nc = E.C.n;
    double* o = out + (int64_t)l * nc * EV_VALUES;
    const int32_t s = E.lstart[l], len = E.lstart[l + 1] - s;
    // the user's row of relevant items: one binary search in the user table, wave-uniform
    const uint32_t user = (uint32_t)__builtin_amdgcn_readfirstlane(E.key0[s]);
    int32_t lo = 0, hi = E.n_users;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (E.tuser[mid] < user) lo = mid + 1; else hi = mid;
    }
    if (lo >= E.n_users || E.tuser[lo] != user) {
        if (lane < nc * EV_VALUES) o[lane] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    const int32_t rs = E.tstart[lo], cnt = E.tstart[lo + 1] - rs;
    const uint32_t* row = E.titem + rs;

    double ap[FY_EVAL_MAX_CUTOFFS], dcg[FY_EVAL_MAX_CUTOFFS];
    int32_t hits[FY_EVAL_MAX_CUTOFFS];
#pragma unroll
    for (int c = 0; c < FY_EVAL_MAX_CUTOFFS; c++) { ap[c] = 0.0; dcg[c] = 0.0; hits[c] = 0; }
    int32_t carry = 0, first = 0;                               // hits in front of the chunk; first hit position (1-based), 0 = none yet
    const int32_t lim = min(len, E.C.last);
    for (int32_t base = 0; base < lim; base += 64) {            // wave-uniform trip count
        const int32_t p0 = base + lane;
        int32_t j = -1;
        if (p0 < lim) {
            const uint32_t it = (uint32_t)E.key1[s + p0];
            int32_t a = 0, b = cnt;
            while (a < b) {
                const int32_t mid = (a + b) >> 1;
                if (row[mid] < it) a = mid + 1; else b = mid;
            }
            if (a < cnt && row[a] == it) j = a;
        }
        const unsigned long long mask = __ballot(j >= 0);
        if (j >= 0) {
            const int32_t p = p0 + 1;
            const double h = (double)(carry + __popcll(mask & ((2ull << lane) - 1ull))) / (double)p;     // hits up to and at this lane
            const double g = (E.tgain ? E.tgain[rs + j] : 1.0) * ev_disc[p0];
#pragma unroll
            for (int c = 0; c < FY_EVAL_MAX_CUTOFFS; c++)
                if (c < nc && p <= E.C.at[c]) { ap[c] += h; dcg[c] += g; }
        }
#pragma unroll
        for (int c = 0; c < FY_EVAL_MAX_CUTOFFS; c++)
            if (c < nc) {
                const int32_t room = E.C.at[c] - base;          // positions of this chunk inside the cutoff
                const unsigned long long clip = room >= 64 ? ~0ull : room <= 0 ? 0ull : (1ull << room) - 1ull;
                hits[c] += __popcll(mask & clip);
            }
        if (!first && mask) first = base + __ffsll((unsigned long long)mask);
        carry += __popcll(mask);
    }
#pragma unroll
    for (int c = 0; c < FY_EVAL_MAX_CUTOFFS; c++) {
        const double a = ev_wave_sum(ap[c]), d = ev_wave_sum(dcg[c]);
        if (lane == 0 && c < nc) {
            const int32_t N = E.C.at[c];
            o[c * EV_VALUES + 0] = (double)hits[c];
            o[c * EV_VALUES + 1] = (double)hits[c] / (double)cnt;
            o[c * EV_VALUES + 2] = a / (double)min(cnt, N);
            o[c * EV_VALUES + 3] = first && first <= N ? 1.0 / (double)first : 0.0;
            o[c * EV_VALUES + 4] = d / E.idcg[(int64_t)lo * nc + c];
        }
    }
}

// ---------------------------------------------------------------- the sums, in a fixed order
// Slice b of EV_SLICES takes lists [b * per, (b + 1) * per); thread t of its block the lists t, t + 256, ... of the slice; the threads'
// sums meet in the xor butterfly, the four waves' in wave order, the slices' in slice order (k_ev_sum_slices).
constexpr int EV_SLICES = 64;
constexpr int EV_NF = 4 * FY_EVAL_MAX_CUTOFFS;       // fp64 sums: [recall, AP, RR, nDCG][cutoff]
constexpr int EV_NI = 2 * FY_EVAL_MAX_CUTOFFS + 1;   // integer sums: [hits, users_hit][cutoff], evaluated lists

__global__ void __launch_bounds__(256) k_ev_sum_lists(int32_t n_lists, int32_t per, int nc, const double* __restrict__ vals, double* __restrict__ part_f,
                                                      long long* __restrict__ part_i) {
    const int32_t lo = min(n_lists, (int32_t)blockIdx.x * per), hi = min(n_lists, lo + per);
    double f[EV_NF];
    long long n[EV_NI];
#pragma unroll
    for (int k = 0; k < EV_NF; k++) f[k] = 0.0;
#pragma unroll
    for (int k = 0; k < EV_NI; k++) n[k] = 0;
    for (int32_t l = lo + (int32_t)threadIdx.x; l < hi; l += 256) {
        const double* v = vals + (int64_t)l * nc * EV_VALUES;
        if (v[0] != v[0]) continue;                              // not evaluated
        n[EV_NI - 1]++;
#pragma unroll
        for (int c = 0; c < FY_EVAL_MAX_CUTOFFS; c++)
            if (c < nc) {
                const long long h = (long long)v[c * EV_VALUES];
                n[c] += h;
                n[FY_EVAL_MAX_CUTOFFS + c] += h > 0;
#pragma unroll
                for (int q = 0; q < 4; q++) f[q * FY_EVAL_MAX_CUTOFFS + c] += v[c * EV_VALUES + 1 + q];
            }
    }
    __shared__ double sh_f[4][EV_NF];
    __shared__ long long sh_i[4][EV_NI];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < EV_NF; k++) {
        const double s = ev_wave_sum(f[k]);
        if (lane == 0) sh_f[wv][k] = s;
    }
#pragma unroll
    for (int k = 0; k < EV_NI; k++) {
        long long s = n[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) sh_i[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < EV_NF) part_f[blockIdx.x * EV_NF + threadIdx.x] = ((sh_f[0][threadIdx.x] + sh_f[1][threadIdx.x]) + sh_f[2][threadIdx.x]) + sh_f[3][threadIdx.x];
    if (threadIdx.x < EV_NI) part_i[blockIdx.x * EV_NI + threadIdx.x] = sh_i[0][threadIdx.x] + sh_i[1][threadIdx.x] + sh_i[2][threadIdx.x] + sh_i[3][threadIdx.x];
}
__global__ void k_ev_sum_slices(const double* __restrict__ part_f, const long long* __restrict__ part_i, double* __restrict__ sum_f, long long* __restrict__ sum_i) {
    const int k = threadIdx.x;
    if (k < EV_NF) {
        double s = 0.0;
        for (int b = 0; b < EV_SLICES; b++) s += part_f[b * EV_NF + k];
        sum_f[k] = s;
    }
    if (k < EV_NI) {
        long long s = 0;
        for (int b = 0; b < EV_SLICES; b++) s += part_i[b * EV_NI + k];
        sum_i[k] = s;
    }
}

// ---------------------------------------------------------------- rating errors of an estimates result (fy_eval_estimates)
// The siblings of k_ev_sum_lists / k_ev_sum_slices for one row per PAIR: the per-pair terms are formed where they are summed (no
// per-pair values in HBM), the order is the same fixed one: slice b of EV_SLICES takes rows [b * per, (b + 1) * per), thread t of its
// block the rows t, t + 256, ... of the slice, the threads meet in the xor butterfly, the four waves in wave order, the slices in slice
// order.  Integer sums: rows per status [0 .. 7], rows in the sums [8], OK rows with a truth score that is not finite [9], rows whose
// (user, item) is not the truth entry's [10].
constexpr int EV_ERR_NF = 3;         // sum |e|, sum e^2, sum e
constexpr int EV_ERR_NI = 11;
struct EvalErrors {
    int32_t n, per;
    const int32_t* key0;             // the estimates' rows
    const int32_t* key1;
    const float* value;
    const int32_t* aux;
    const int32_t* t_user;           // the truth entries of the same rows (already offset)
    const int32_t* t_item;
    const float* t_score;
    int32_t has_clamp;
    double lo, hi;
};
__global__ void __launch_bounds__(256) k_ev_sum_errors(EvalErrors E, double* __restrict__ part_f, long long* __restrict__ part_i) {
    const int32_t lo = min(E.n, (int32_t)blockIdx.x * E.per), hi = min(E.n, lo + E.per);
    double f[EV_ERR_NF] = {0.0, 0.0, 0.0};
    long long n[EV_ERR_NI];
#pragma unroll
    for (int k = 0; k < EV_ERR_NI; k++) n[k] = 0;
    for (int32_t r = lo + (int32_t)threadIdx.x; r < hi; r += 256) {
        const int32_t status = E.aux[r] & 7;
#pragma unroll
        for (int q = 0; q < 8; q++) n[q] += status == q;
        n[10] += E.key0[r] != E.t_user[r] || E.key1[r] != E.t_item[r];
        if (status != FY_ESTIMATE_OK) continue;
        const double truth = (double)E.t_score[r];
        if (!(fabs(truth) <= 1.7976931348623157e308)) {          // NaN or infinite
            n[9]++;
            continue;
        }
        double est = (double)E.value[r];
        if (E.has_clamp) est = est < E.lo ? E.lo : est > E.hi ? E.hi : est;
        const double e = est - truth;
        n[8]++;
        f[0] += fabs(e);
        f[1] += __dmul_rn(e, e);
        f[2] += e;
    }
    __shared__ double sh_f[4][EV_ERR_NF];
    __shared__ long long sh_i[4][EV_ERR_NI];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < EV_ERR_NF; k++) {
        const double s = ev_wave_sum(f[k]);
        if (lane == 0) sh_f[wv][k] = s;
    }
#pragma unroll
    for (int k = 0; k < EV_ERR_NI; k++) {
        long long s = n[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) sh_i[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < EV_ERR_NF) part_f[blockIdx.x * EV_ERR_NF + threadIdx.x] = ((sh_f[0][threadIdx.x] + sh_f[1][threadIdx.x]) + sh_f[2][threadIdx.x]) + sh_f[3][threadIdx.x];
    if (threadIdx.x < EV_ERR_NI) part_i[blockIdx.x * EV_ERR_NI + threadIdx.x] = sh_i[0][threadIdx.x] + sh_i[1][threadIdx.x] + sh_i[2][threadIdx.x] + sh_i[3][threadIdx.x];
}
__global__ void k_ev_sum_error_slices(const double* __restrict__ part_f, const long long* __restrict__ part_i, double* __restrict__ sum_f, long long* __restrict__ sum_i) {
    const int k = threadIdx.x;
    if (k < EV_ERR_NF) {
        double s = 0.0;
        for (int b = 0; b < EV_SLICES; b++) s += part_f[b * EV_ERR_NF + k];
        sum_f[k] = s;
    }
    if (k < EV_ERR_NI) {
        long long s = 0;
        for (int b = 0; b < EV_SLICES; b++) s += part_i[b * EV_ERR_NI + k];
        sum_i[k] = s;
    }
}

__global__ void k_ev_list_users(int32_t n_lists,const int32_t* __restrict__ lstart, const int32_t* __restrict__ key0, int32_t* __restrict__ out) {
    for (int32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < n_lists; l += gridDim.x * blockDim.x) out[l] = key0[lstart[l]];
}

// ---------------------------------------------------------------- coverage: the items among the first `last` rows of every list
constexpr uint64_t EV_NO_ITEM = 1ull << 32;
__global__ void k_ev_cover_keys(int32_t n, const int32_t* __restrict__ key1, const uint32_t* __restrict__ head_incl, const int32_t* __restrict__ lstart,
                                int32_t last, uint64_t* __restrict__ keys) {
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x)
        keys[t] = t - lstart[head_incl[t] - 1] < last ? (uint64_t)(uint32_t)key1[t] : EV_NO_ITEM;
}
__global__ void k_ev_count_distinct(int32_t n, const uint64_t* __restrict__ sorted, unsigned long long* __restrict__ count) {
    const int32_t n_up = (n + 63) & ~63;                        // whole waves enter every ballot
    unsigned long long c = 0;
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_up; t += gridDim.x * blockDim.x)
        c += __popcll(__ballot(t < n && sorted[t] != EV_NO_ITEM && (t == 0 || sorted[t] != sorted[t - 1])));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

// heads of the rows of a list result: n_lists, lstart (n_lists + 1) and the inclusive head count per row; synchronises once
struct ListHeads {
    int32_t n_lists = 0;
    DevBuf<uint32_t> head, head_incl;
    DevBuf<int32_t> lstart;
};
void find_lists(Context* ctx, int32_t n, const int32_t* key0, ListHeads& H, DevBuf<uint64_t>* luser_key) {
    if (n == 0) return;
    H.head.alloc(ctx, (size_t)n);
    H.head_incl.alloc(ctx, (size_t)n);
    k_ev_heads<<<small_grid(n), 256, 0, ctx->stream>>>(n, key0, H.head.get());
    FY_KERNEL_CHECK();
    inclusive_scan_u32(ctx, H.head.get(), H.head_incl.get(), (size_t)n);
    H.n_lists = (int32_t)fetch(ctx, H.head_incl.get() + (n - 1));
    if (H.n_lists < 1 || H.n_lists > n) FY_FAIL(FY_ERR_HIP, "list heads: %d lists in %d rows", H.n_lists, n);
    H.lstart.alloc(ctx, (size_t)H.n_lists + 1);
    if (luser_key) luser_key->alloc(ctx, (size_t)H.n_lists);
    k_ev_list_starts<<<small_grid(n), 256, 0, ctx->stream>>>(n, key0, H.head.get(), H.head_incl.get(), H.lstart.get(), luser_key ? luser_key->get() : nullptr);
    FY_KERNEL_CHECK();
}

}  // namespace

// ================================================================ fy_ratings_holdout
void ratings_holdout(Context* ctx, const fy_ratings* R, double fraction, uint64_t seed, fy_ratings** train, fy_ratings** test) {
    if (!(fraction >= 0.0 && fraction <= 1.0)) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "hold-out fraction %g is not in [0, 1]", fraction);
    const int64_t nnz = R->nnz;
    hipStream_t sm = ctx->stream;
    std::unique_ptr<fy_ratings> tr(new fy_ratings), te(new fy_ratings);
    tr->ctx = te->ctx = ctx;
    Holdout S{};
    S.nnz = nnz;
    S.user = R->user.get(); S.item = R->item.get(); S.score = R->score.get();
    S.seed_term = seed * 0x9E3779B97F4A7C15ull;
    S.threshold = (uint64_t)std::floor(fraction * 16777216.0);
    int64_t n_test = 0;
    int grid = 0;
    DevBuf<int64_t> wave_count, wave_incl;
    if (nnz) {
        grid = (int)std::max<int64_t>(1, std::min<int64_t>(8 * (int64_t)ctx->num_cus, ceil_div(nnz, (int64_t)HO_WAVES * 256)));
        const int64_t n_waves = (int64_t)grid * HO_WAVES;
        S.per = round_up(ceil_div(nnz, n_waves), (int64_t)64);
        wave_count.alloc(ctx, (size_t)n_waves);
        wave_incl.alloc(ctx, (size_t)n_waves);
        k_holdout<false><<<grid, HO_BLOCK, 0, sm>>>(S, wave_count.get(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        FY_KERNEL_CHECK();
        inclusive_scan_i64(ctx, wave_count.get(), wave_incl.get(), (size_t)n_waves);
        n_test = fetch(ctx, wave_incl.get() + (n_waves - 1));
    }
    if (n_test < 0 || n_test > nnz) FY_FAIL(FY_ERR_HIP, "hold-out: %lld test entries of %lld", (long long)n_test, (long long)nnz);
    te->nnz = n_test;
    tr->nnz = nnz - n_test;
    for (fy_ratings* o : {tr.get(), te.get()}) {
        o->user.alloc(ctx, (size_t)o->nnz);
        o->item.alloc(ctx, (size_t)o->nnz);
        o->score.alloc(ctx, (size_t)o->nnz);
    }
    if (nnz) {
        k_holdout<true><<<grid, HO_BLOCK, 0, sm>>>(S, nullptr, wave_incl.get(), tr->user.get(), tr->item.get(), tr->score.get(), te->user.get(),
                                                   te->item.get(), te->score.get());
        FY_KERNEL_CHECK();
    }
    ratings_id_bounds(ctx, tr.get());       // the bounds of each side's own contents (synchronises)
    ratings_id_bounds(ctx, te.get());
    sync(ctx);
    *train = tr.release();
    *test = te.release();
}

// ================================================================ fy_result_create_lists
fy_result* result_create_lists(Context* ctx, int64_t n, const int32_t* user, const int32_t* item, const float* value, int location) {
    if (n > INT32_MAX) FY_FAIL(FY_ERR_UNSUPPORTED, "%lld list rows: at most 2^31 - 1", (long long)n);
    std::unique_ptr<fy_result> res(new fy_result);
    res->ctx = ctx;
    res->kind = 2;
    res->n = n;
    res->d_key0.alloc(ctx, (size_t)n);
    res->d_key1.alloc(ctx, (size_t)n);
    res->d_aux.alloc(ctx, (size_t)n);
    res->d_value.alloc(ctx, (size_t)n);
    res->d_aux.zero();
    SyncOnUnwind drain(ctx->stream);        // the caller's arrays are the sources of the queued copies
    if (n) {
        const hipMemcpyKind k = location == FY_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
        FY_HIP(hipMemcpyAsync(res->d_key0.get(), user, (size_t)n * 4, k, ctx->stream));
        FY_HIP(hipMemcpyAsync(res->d_key1.get(), item, (size_t)n * 4, k, ctx->stream));
        FY_HIP(hipMemcpyAsync(res->d_value.get(), value, (size_t)n * 4, k, ctx->stream));
    }
    ListHeads H;
    DevBuf<uint64_t> luser;
    find_lists(ctx, (int32_t)n, res->d_key0.get(), H, &luser);
    if (H.n_lists > 1) {                    // a user with two separate runs of rows heads two lists
        DevBuf<uint64_t> sorted(ctx, (size_t)H.n_lists);
        DevBuf<uint32_t> flag(ctx, 1);
        flag.zero();
        sort_keys_u64(ctx, luser.get(), sorted.get(), (size_t)H.n_lists, 32);
        k_ev_adjacent_equal<<<small_grid(H.n_lists), 256, 0, ctx->stream>>>(H.n_lists, sorted.get(), flag.get());
        FY_KERNEL_CHECK();
        if (fetch(ctx, flag.get())) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "the rows of a user form two separate runs: lists must be grouped by user");
    }
    sync(ctx);
    res->st.recs = n;
    res->st.users_scored = H.n_lists;
    return res.release();
}

// ================================================================ fy_eval_prepare
fy_eval* eval_prepare(Context* ctx, const fy_eval_params* p, const fy_ratings* T) {
    if (p->n_cutoffs < 1 || p->n_cutoffs > FY_EVAL_MAX_CUTOFFS) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "n_cutoffs %d is not in [1, %d]", p->n_cutoffs, FY_EVAL_MAX_CUTOFFS);
    for (int c = 0; c < p->n_cutoffs; c++)
        if (p->cutoffs[c] < 1 || p->cutoffs[c] > FY_EVAL_MAX_CUTOFF || (c && p->cutoffs[c] <= p->cutoffs[c - 1]))
            FY_FAIL(FY_ERR_INVALID_ARGUMENT, "cutoffs must be strictly ascending and in [1, %d] (cutoff %d is %d)", FY_EVAL_MAX_CUTOFF, c, p->cutoffs[c]);
    if (p->gain != FY_EVAL_GAIN_BINARY && p->gain != FY_EVAL_GAIN_LINEAR && p->gain != FY_EVAL_GAIN_EXP2) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "gain %d is no FY_EVAL_GAIN_*", p->gain);
    if (p->flags & ~FY_EVAL_COVERAGE) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "unknown evaluator flags 0x%x", p->flags);
    if (p->relevance_threshold != p->relevance_threshold) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "relevance_threshold is NaN");
    if (p->gain != FY_EVAL_GAIN_BINARY && !(p->relevance_threshold > 0.0)) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "a graded gain needs relevance_threshold > 0 (got %g)", p->relevance_threshold);
    if (T->nnz > INT32_MAX) FY_FAIL(FY_ERR_UNSUPPORTED, "%lld test ratings: at most 2^31 - 1", (long long)T->nnz);
    const int32_t n = (int32_t)T->nnz;
    const int nc = p->n_cutoffs, last = p->cutoffs[nc - 1];
    const bool graded = p->gain != FY_EVAL_GAIN_BINARY;
    hipStream_t sm = ctx->stream;
    std::unique_ptr<fy_eval> E(new fy_eval);
    E->ctx = ctx;
    E->p = *p;
    for (int c = nc; c < FY_EVAL_MAX_CUTOFFS; c++) E->p.cutoffs[c] = 0;

    // the discount table 1 / log2(p + 1) and its running sum, fp64, once
    std::vector<double> h_disc((size_t)last), h_cum((size_t)last + 1);
    h_cum[0] = 0.0;
    for (int k = 0; k < last; k++) {
        h_disc[(size_t)k] = 1.0 / std::log2((double)k + 2.0);
        h_cum[(size_t)k + 1] = h_cum[(size_t)k] + h_disc[(size_t)k];
    }
    DevBuf<double> cum(ctx, (size_t)last + 1);
    E->discount.alloc(ctx, (size_t)last);
    SyncOnUnwind drain(sm);                 // the tables above are the sources of the queued uploads
    h2d(ctx, E->discount.get(), h_disc.data(), (size_t)last);
    h2d(ctx, cum.get(), h_cum.data(), (size_t)last + 1);

    int32_t m = 0, nu = 0;
    DevBuf<uint64_t> ckey, gkey;
    DevBuf<uint32_t> gpos;
    DevBuf<double> cgain;
    if (n) {
        DevBuf<uint64_t> keys(ctx, (size_t)n), skeys(ctx, (size_t)n);
        DevBuf<uint32_t> pos(ctx, (size_t)n), spos(ctx, (size_t)n), rel(ctx, (size_t)n), rel_incl(ctx, (size_t)n), flag(ctx, 1);
        flag.zero();
        k_ev_pack<<<small_grid(n), 256, 0, sm>>>(n, T->user.get(), T->item.get(), keys.get(), pos.get());
        FY_KERNEL_CHECK();
        sort_pairs_u64_u32(ctx, keys.get(), skeys.get(), pos.get(), spos.get(), (size_t)n);
        k_ev_relevant<<<small_grid(n), 256, 0, sm>>>(n, skeys.get(), spos.get(), T->score.get(), p->relevance_threshold, rel.get(), flag.get());
        FY_KERNEL_CHECK();
        inclusive_scan_u32(ctx, rel.get(), rel_incl.get(), (size_t)n);
        uint32_t h_dup = 0, h_m = 0;
        d2h(ctx, &h_dup, flag.get(), 1);
        d2h(ctx, &h_m, rel_incl.get() + (n - 1), 1);
        sync(ctx);
        if (h_dup) FY_FAIL(FY_ERR_DUPLICATE_RATING, "the test ratings hold a (user, item) twice");
        m = (int32_t)h_m;
        if (m < 0 || m > n) FY_FAIL(FY_ERR_HIP, "evaluator: %d relevant entries of %d", m, n);
        if (m) {
            ckey.alloc(ctx, (size_t)m);
            if (graded) { cgain.alloc(ctx, (size_t)m); gkey.alloc(ctx, (size_t)m); gpos.alloc(ctx, (size_t)m); }
            k_ev_compact<<<small_grid(n), 256, 0, sm>>>(n, skeys.get(), spos.get(), T->score.get(), rel.get(), rel_incl.get(), p->gain, ckey.get(),
                                                        cgain.get(), gkey.get(), gpos.get());
            FY_KERNEL_CHECK();
        }
    }
    E->n_entries = m;
    if (m) {
        DevBuf<uint32_t> head(ctx, (size_t)m), head_incl(ctx, (size_t)m);
        k_ev_user_heads<<<small_grid(m), 256, 0, sm>>>(m, ckey.get(), head.get());
        FY_KERNEL_CHECK();
        inclusive_scan_u32(ctx, head.get(), head_incl.get(), (size_t)m);
        nu = (int32_t)fetch(ctx, head_incl.get() + (m - 1));
        if (nu < 1 || nu > m) FY_FAIL(FY_ERR_HIP, "evaluator: %d users over %d relevant entries", nu, m);
        E->user.alloc(ctx, (size_t)nu);
        E->start.alloc(ctx, (size_t)nu + 1);
        E->item.alloc(ctx, (size_t)m);
        E->idcg.alloc(ctx, (size_t)nu * nc);
        k_ev_table<<<small_grid(m), 256, 0, sm>>>(m, ckey.get(), head.get(), head_incl.get(), E->user.get(), E->start.get(), E->item.get());
        FY_KERNEL_CHECK();
        DevBuf<double> sorted_gain;
        if (graded) {
            DevBuf<uint64_t> gkey_sorted(ctx, (size_t)m);
            DevBuf<uint32_t> order(ctx, (size_t)m);
            sorted_gain.alloc(ctx, (size_t)m);
            sort_pairs_u64_u32(ctx, gkey.get(), gkey_sorted.get(), gpos.get(), order.get(), (size_t)m);
            k_ev_gather_gain<<<small_grid(m), 256, 0, sm>>>(m, cgain.get(), order.get(), sorted_gain.get());
            FY_KERNEL_CHECK();
            E->gain = std::move(cgain);
        }
        Cutoffs C{};
        C.n = nc; C.last = last;
        for (int c = 0; c < nc; c++) C.at[c] = p->cutoffs[c];
        k_ev_idcg<<<(int)ceil_div((int64_t)nu, (int64_t)4), 256, 0, sm>>>(nu, E->start.get(), graded ? sorted_gain.get() : nullptr, E->discount.get(), cum.get(), C,
                                                                         E->idcg.get());
        FY_KERNEL_CHECK();
    }
    E->n_users = nu;
    sync(ctx);
    return E.release();
}

// ================================================================ fy_eval_lists
void eval_lists(fy_eval* E, fy_result* R, fy_eval_sums* out, int32_t* per_user_id, double* per_user) {
    Context* ctx = E->ctx;
    if (R->n > INT32_MAX) FY_FAIL(FY_ERR_UNSUPPORTED, "%lld list rows: at most 2^31 - 1", (long long)R->n);
    const int32_t n = (int32_t)R->n;
    const int nc = E->p.n_cutoffs, last = E->p.cutoffs[nc - 1];
    hipStream_t sm = ctx->stream;
    fy_eval_sums S{};
    S.n_cutoffs = nc;
    for (int c = 0; c < nc; c++) S.cutoffs[c] = E->p.cutoffs[c];
    S.relevant_users = E->n_users;
    S.relevant_entries = E->n_entries;
    S.distinct_items = (E->p.flags & FY_EVAL_COVERAGE) ? 0 : -1;
    EventTimer timer(ctx);
    const size_t span = timer.begin();
    ListHeads H;
    find_lists(ctx, n, R->d_key0.get(), H, nullptr);
    const int32_t L = H.n_lists;
    S.lists = L;
    if (L) {
        DevBuf<double> vals(ctx, (size_t)L * nc * EV_VALUES), part_f(ctx, (size_t)EV_SLICES * EV_NF), sum_f(ctx, EV_NF);
        DevBuf<long long> part_i(ctx, (size_t)EV_SLICES * EV_NI), sum_i(ctx, EV_NI);
        DevBuf<int32_t> list_user;
        DevBuf<unsigned long long> distinct;
        EvalLists A{};
        A.n_lists = L;
        A.lstart = H.lstart.get();
        A.key0 = R->d_key0.get(); A.key1 = R->d_key1.get();
        A.n_users = E->n_users;
        A.tuser = E->user.get(); A.tstart = E->start.get(); A.titem = E->item.get();
        A.tgain = E->p.gain != FY_EVAL_GAIN_BINARY && E->n_entries ? E->gain.get() : nullptr;
        A.idcg = E->idcg.get();
        A.discount = E->discount.get();
        A.C.n = nc; A.C.last = last;
        for (int c = 0; c < nc; c++) A.C.at[c] = E->p.cutoffs[c];
        k_ev_metrics<<<(int)ceil_div((int64_t)L, (int64_t)4), 256, (size_t)last * sizeof(double), sm>>>(A, vals.get());
        FY_KERNEL_CHECK();
        k_ev_sum_lists<<<EV_SLICES, 256, 0, sm>>>(L, (int32_t)ceil_div((int64_t)L, (int64_t)EV_SLICES), nc, vals.get(), part_f.get(), part_i.get());
        FY_KERNEL_CHECK();
        k_ev_sum_slices<<<1, 64, 0, sm>>>(part_f.get(), part_i.get(), sum_f.get(), sum_i.get());
        FY_KERNEL_CHECK();
        if (E->p.flags & FY_EVAL_COVERAGE) {
            DevBuf<uint64_t> keys(ctx, (size_t)n), sorted(ctx, (size_t)n);
            distinct.alloc(ctx, 1);
            distinct.zero();
            k_ev_cover_keys<<<small_grid(n), 256, 0, sm>>>(n, R->d_key1.get(), H.head_incl.get(), H.lstart.get(), last, keys.get());
            FY_KERNEL_CHECK();
            sort_keys_u64(ctx, keys.get(), sorted.get(), (size_t)n, 33);
            k_ev_count_distinct<<<small_grid(n), 256, 0, sm>>>(n, sorted.get(), distinct.get());
            FY_KERNEL_CHECK();
        }
        if (per_user_id) {
            list_user.alloc(ctx, (size_t)L);
            k_ev_list_users<<<small_grid(L), 256, 0, sm>>>(L, H.lstart.get(), R->d_key0.get(), list_user.get());
            FY_KERNEL_CHECK();
        }
        timer.end(span);
        double h_f[EV_NF];
        long long h_i[EV_NI];
        unsigned long long h_distinct = 0;
        d2h(ctx, h_f, sum_f.get(), EV_NF);
        d2h(ctx, h_i, sum_i.get(), EV_NI);
        if (E->p.flags & FY_EVAL_COVERAGE) d2h(ctx, &h_distinct, distinct.get(), 1);
        if (per_user_id) d2h(ctx, per_user_id, list_user.get(), (size_t)L);
        if (per_user) d2h(ctx, per_user, vals.get(), (size_t)L * nc * EV_VALUES);
        sync(ctx);
        for (int c = 0; c < nc; c++) {
            S.hits[c] = h_i[c];
            S.users_hit[c] = h_i[FY_EVAL_MAX_CUTOFFS + c];
            S.recall[c] = h_f[0 * FY_EVAL_MAX_CUTOFFS + c];
            S.ap[c] = h_f[1 * FY_EVAL_MAX_CUTOFFS + c];
            S.rr[c] = h_f[2 * FY_EVAL_MAX_CUTOFFS + c];
            S.ndcg[c] = h_f[3 * FY_EVAL_MAX_CUTOFFS + c];
        }
        S.users_evaluated = h_i[EV_NI - 1];
        if (E->p.flags & FY_EVAL_COVERAGE) S.distinct_items = (int64_t)h_distinct;
    } else {
        timer.end(span);
        sync(ctx);
    }
    S.lists_without_relevant = S.lists - S.users_evaluated;
    S.ms = timer.total_ms();
    *out = S;
}

// ================================================================ fy_eval_estimates
void eval_estimates(Context* ctx, fy_result* R, const fy_ratings* T, const fy_eval_error_params* p, fy_eval_errors* out) {
    if (p && p->has_clamp && !(p->clamp_lo <= p->clamp_hi)) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "clamp [%g, %g]: the bounds must be numbers with lo <= hi", p->clamp_lo, p->clamp_hi);
    if (R->n > INT32_MAX) FY_FAIL(FY_ERR_UNSUPPORTED, "%lld estimate rows: at most 2^31 - 1", (long long)R->n);
    const int32_t n = (int32_t)R->n;
    const int64_t off = R->est.pair_offset;
    if (off < 0 || off + n > T->nnz)
        FY_FAIL(FY_ERR_INVALID_ARGUMENT, "the estimates are the pairs %lld .. %lld of their list, `truth` holds %lld entries", (long long)off, (long long)(off + n), (long long)T->nnz);
    hipStream_t sm = ctx->stream;
    fy_eval_errors S{};
    S.pairs = n;
    EventTimer timer(ctx);
    const size_t span = timer.begin();
    if (n) {
        DevBuf<double> part_f(ctx, (size_t)EV_SLICES * EV_ERR_NF), sum_f(ctx, EV_ERR_NF);
        DevBuf<long long> part_i(ctx, (size_t)EV_SLICES * EV_ERR_NI), sum_i(ctx, EV_ERR_NI);
        EvalErrors E{};
        E.n = n;
        E.per = (int32_t)ceil_div((int64_t)n, (int64_t)EV_SLICES);
        E.key0 = R->d_key0.get(); E.key1 = R->d_key1.get(); E.value = R->d_value.get(); E.aux = R->d_aux.get();
        E.t_user = T->user.get() + off; E.t_item = T->item.get() + off; E.t_score = T->score.get() + off;
        E.has_clamp = p && p->has_clamp;
        E.lo = E.has_clamp ? p->clamp_lo : 0.0;
        E.hi = E.has_clamp ? p->clamp_hi : 0.0;
        k_ev_sum_errors<<<EV_SLICES, 256, 0, sm>>>(E, part_f.get(), part_i.get());
        FY_KERNEL_CHECK();
        k_ev_sum_error_slices<<<1, 64, 0, sm>>>(part_f.get(), part_i.get(), sum_f.get(), sum_i.get());
        FY_KERNEL_CHECK();
        timer.end(span);
        double h_f[EV_ERR_NF];
        long long h_i[EV_ERR_NI];
        d2h(ctx, h_f, sum_f.get(), EV_ERR_NF);
        d2h(ctx, h_i, sum_i.get(), EV_ERR_NI);
        sync(ctx);
        if (h_i[10]) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "%lld rows of the estimates name another (user, item) than the entry of `truth` at their position", h_i[10]);
        for (int q = 0; q < 8; q++) S.by_status[q] = h_i[q];
        S.estimated = h_i[8];
        S.truth_not_finite = h_i[9];
        S.sum_abs = h_f[0];
        S.sum_sq = h_f[1];
        S.sum_err = h_f[2];
    } else {
        timer.end(span);
        sync(ctx);
    }
    S.ms = timer.total_ms();
    *out = S;
}

}  // namespace fy
