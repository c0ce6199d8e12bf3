// fy_itemsim_kernels.hpp -- device code the two item-similarity translation units share (fy_itemsim.hip: the full build,
// fy_itemsim_request.hip: rows on request): the measures' finishing functions, the composite key of a candidate in its two
// encodings, the running top-K in LDS (append / select / cut / finish), the candidate test of a row kernel's accumulator, the one
// compact kernel and the merge of a row's per-chunk lists.  What a measure is and which template it instantiates: fy_itemsim_plan.hpp.
#pragma once
#include "fy_common.hpp"
#include "fy_itemsim_plan.hpp"

namespace fy {

// One function per measure, fp64; the emitted similarity is the (float) of it.  d = the accumulated dot product, a_i / a_j = the
// two items' norms of the table (the count measures: number of raters; Euclidean: sum r^2), N = number of users.
__device__ __forceinline__ double isim_finish_product(double d, double inv_i, double inv_j) { return d * inv_i * inv_j; }   // cosine on raw ratings: inv = 1 / ||r||
__device__ __forceinline__ double isim_finish_tanimoto(double d, double ai, double aj) { return d / (ai + aj - d); }
__device__ __forceinline__ double isim_finish_city_block(double d, double ai, double aj) { return 1.0 / (1.0 + ai + aj - 2.0 * d); }
__device__ __forceinline__ double isim_finish_euclidean(double d, double ai, double aj) { return 1.0 / (1.0 + sqrt(fmax(0.0, ai - 2.0 * d + aj))); }
__device__ __forceinline__ double isim_xlogx(double x) { return x == 0.0 ? 0.0 : x * log(x); }
// Mahout's LogLikelihood.logLikelihoodRatio on unnormalised entropies H(x...) = xlogx(sum x) - sum xlogx(x)
__device__ __forceinline__ double isim_finish_loglikelihood(double d, double ai, double aj, double N) {
    const double k11 = d, k12 = aj - d, k21 = ai - d, k22 = N - ai - aj + d;
    const double row_e = isim_xlogx(k11 + k12 + k21 + k22) - isim_xlogx(k11 + k12) - isim_xlogx(k21 + k22);
    const double col_e = isim_xlogx(k11 + k12 + k21 + k22) - isim_xlogx(k11 + k21) - isim_xlogx(k12 + k22);
    const double mat_e = isim_xlogx(k11 + k12 + k21 + k22) - isim_xlogx(k11) - isim_xlogx(k12) - isim_xlogx(k21) - isim_xlogx(k22);
    const double llr = row_e + col_e < mat_e ? 0.0 : 2.0 * (row_e + col_e - mat_e);
    return 1.0 - 1.0 / (1.0 + llr);
}
template <int M>
__device__ __forceinline__ double isim_finish(double d, double ai, double aj, double N) {
    if constexpr (M == FY_SIMILARITY_TANIMOTO_COEFFICIENT) return isim_finish_tanimoto(d, ai, aj);
    else if constexpr (M == FY_SIMILARITY_LOGLIKELIHOOD) return isim_finish_loglikelihood(d, ai, aj, N);
    else if constexpr (M == FY_SIMILARITY_CITY_BLOCK) return isim_finish_city_block(d, ai, aj);
    else {
        static_assert(M == FY_SIMILARITY_EUCLIDEAN_DISTANCE, "cosine, co-occurrence and Pearson: the dot product is the similarity");
        return isim_finish_euclidean(d, ai, aj);
    }
}

// A candidate is one 64-bit composite: similarity key << 32 | (0x7FFFFFFF - raw item id), so that descending composites are
// descending similarities with ties by ascending item id, all distinct.  The key has two encodings; a list holds ONE of them:
//   * ordered: fy_order_key, any sign -- the row kernels (full build, request), their per-chunk lists and k_isim_merge;
//   * positive: the float's own bits, which order like the floats only for similarities > 0 -- the symmetric build (sweep, finish, redo).
__device__ __forceinline__ uint64_t isim_composite(uint32_t key, int32_t raw_id) { return ((uint64_t)key << 32) | (uint32_t)(0x7FFFFFFF - raw_id); }
__device__ __forceinline__ int32_t isim_composite_item(uint64_t c) { return 0x7FFFFFFF - (int32_t)(uint32_t)c; }
__device__ __forceinline__ float isim_composite_sim_ordered(uint64_t c) { return fy_order_unkey((uint32_t)(c >> 32)); }
__device__ __forceinline__ uint32_t isim_positive_key(float s) { return __float_as_uint(s); }
__device__ __forceinline__ float isim_composite_sim_positive(uint64_t c) { return __uint_as_float((uint32_t)(c >> 32)); }

constexpr int ISIM_CAP = 2048;      // candidate buffer (LDS)
constexpr int ISIM_MAX_K = 1024;
constexpr int ISIM_SAMPLE = 256;       // columns sampled for the first threshold guess of a row
constexpr int ISIM_SAMPLE_RANK = 5;    // ... whose 5th largest is the guess (expected: ~5 * columns / 256 values above it)

struct ISimEpilogue {
    const int32_t* __restrict__ rank_item_raw;
    int32_t K;
    int32_t exclude_self;
    int32_t has_threshold;
    float threshold;
    int32_t rank, world;     // this launch builds rows rank, rank + world, ...
    int32_t* __restrict__ out_cnt;     // [rows_mine]
    int32_t* __restrict__ out_other;   // [rows_mine * K]
    float* __restrict__ out_sim;       // [rows_mine * K]
    // packed row kernel: the accumulators hold sum_v r_vi r_vj (exact in fp64 for fp16-exact ratings); cosine = that times
    // inv_norm[i] inv_norm[j] (rank order).  nullptr: the weights were divided by the norms beforehand.
    const double* __restrict__ inv_norm;
    // the measures with a finishing function (Tanimoto, log-likelihood, city block, Euclidean distance): a_i in rank order, and N
    const double* __restrict__ aux;
    double n_cols;
    // per (row, chunk) item: its top K as (order key << 32 | ~raw item id), descending
    int32_t* __restrict__ part_cnt;    // [rows_mine * nch]
    uint64_t* __restrict__ part;       // [rows_mine * nch * K]
    int32_t heavy_rows;                // leading rows of the launch that are split by chunk
    int32_t n_items;                   // heavy_rows * nch + (rows - heavy_rows)
    int32_t cap;                       // candidate buffer entries in LDS (power of two, >= 2 K, <= ISIM_CAP)
};

// Cuts the n candidates in LDS down to (at least) the K best without sorting them: two 256-bin histogram levels over the
// order keys (bits 31..24, then 23..16) locate a 16-bit key prefix T with  #(key >= T) >= K  and  #(key >= T + 1 prefix) < K;
// everything below T goes.  ~8 barriers instead of the 66 of a 2048-element bitonic sort (rocprof: the sorts were half
// of the kernel).  Returns the new count through sh_cnt and the new threshold through sh_tau; all threads call it.
// Ties inside the last prefix all stay, so the result may hold more than K entries -- if it would not fit behind the next
// streaming step the caller falls back to the exact sort.
__device__ __forceinline__ void isim_select(uint64_t* cand, int n, int K, uint32_t* hist, uint32_t* sh_cnt, uint32_t* sh_tau,
                                            uint32_t* sh_aux) {
    const int tid = threadIdx.x, nt = blockDim.x;
    if (n <= K) {   // block-uniform: nothing to cut
        return;
    }
    uint32_t prefix = 0, above = 0;
    for (int level = 0; level < 2; level++) {
        const int shift = level == 0 ? 24 : 16;
        for (int b = tid; b < 256; b += nt) hist[b] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += nt) {
            const uint32_t key = (uint32_t)(cand[i] >> 32);
            if (level == 0 || (key >> 24) == (prefix >> 24)) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t cum = above;
            int b = 255;
            for (; b > 0; b--) {
                if (cum + hist[b] >= (uint32_t)K) break;
                cum += hist[b];
            }
            sh_aux[0] = prefix | ((uint32_t)b << shift);
            sh_aux[1] = cum;
        }
        __syncthreads();
        prefix = sh_aux[0];
        above = sh_aux[1];
        __syncthreads();
    }
    // keep key >= prefix (in place: all reads happen before the first write)
    uint64_t mine[ISIM_CAP / 256];
    int have = 0;
    for (int i = tid; i < n; i += nt) {
        const uint64_t c = cand[i];
        if ((uint32_t)(c >> 32) >= prefix && have < ISIM_CAP / 256) mine[have++] = c;
    }
    __syncthreads();
    if (tid == 0) *sh_cnt = 0;
    __syncthreads();
    for (int k = 0; k < have; k++) cand[atomicAdd(sh_cnt, 1u)] = mine[k];
    if (tid == 0) *sh_tau = prefix;
    __syncthreads();
}

// buffer (nearly) full: keep the K best (plus ties inside the last key prefix); exact sort when even that does not make room
__device__ __forceinline__ void isim_cut(uint64_t* cand, int K, int cap, uint32_t* hist, uint32_t* sh_cnt, uint32_t* sh_tau, uint32_t* sh_aux) {
    const int tid = threadIdx.x;
    isim_select(cand, (int)*sh_cnt, K, hist, sh_cnt, sh_tau, sh_aux);
    if (*sh_cnt + min((uint32_t)blockDim.x, (uint32_t)cap / 2) > (uint32_t)cap) {   // massive ties inside one key prefix (block-uniform)
        const int n = (int)*sh_cnt;
        __syncthreads();
        for (int i = n + tid; i < cap; i += blockDim.x) cand[i] = 0ull;
        __syncthreads();
        fy_bitonic_desc(cand, cap);
        if (tid == 0) {
            *sh_cnt = (uint32_t)min(n, K);
            if (n >= K) *sh_tau = (uint32_t)(cand[K - 1] >> 32);   // inclusive: a later tie with a smaller item id still wins
        }
        __syncthreads();
    }
}

// similarity of (row, col) from the accumulator a.  M = FY_SIMILARITY_COSINE stands for the three measures whose dot product IS the
// similarity (cosine, co-occurrence, Pearson: the norms are in the weights, or -- packed cosine -- in inv_norm); the others finish
// through isim_finish<M>.  For those an untouched accumulator is not similarity 0, so a pair nobody co-rated (a == 0; exact: the
// weights are positive) reads as NaN, which passes no comparison.
template <int M>
__device__ __forceinline__ float isim_row_value(const ISimEpilogue& E, double a, double row_term, int col) {
    if constexpr (M == FY_SIMILARITY_COSINE) return E.inv_norm ? (float)isim_finish_product(a, row_term, E.inv_norm[col]) : (float)a;
    else return a != 0.0 ? (float)isim_finish<M>(a, row_term, E.aux[col], E.n_cols) : __builtin_nanf("");
}

// the row's own term of isim_row_value: a_i of a finishing measure, 1 / ||r_.i|| of the packed cosine, else nothing
template <int M>
__device__ __forceinline__ double isim_row_scale(const ISimEpilogue& E, int row) {
    return M != FY_SIMILARITY_COSINE ? E.aux[row] : E.inv_norm ? E.inv_norm[row] : 1.0;
}

// The candidate test of a row kernel: the similarity of (row, col) from the accumulator a, the job's threshold (none: > 0), the
// diagonal.  Returns whether the job accepts the pair, and its ordered key (meaningful either way: the running threshold compares it).
template <int M>
__device__ __forceinline__ bool isim_candidate(const ISimEpilogue& E, double a, double row_term, int row, int col, uint32_t& key) {
    const float s = isim_row_value<M>(E, a, row_term, col);
    bool ok = E.has_threshold ? (s >= E.threshold) : (s > 0.0f);
    if (E.exclude_self && col == row) ok = false;
    key = fy_order_key(s);
    return ok;
}

// Appends the composites of the lanes that `want` to the candidate buffer in LDS with one atomic per wave; every lane of the wave
// calls it.  Returns whether this lane's composite was stored.  BOUNDED (k_cooc_itemsim): the count moves past `cap` when the buffer
// is full and the entry is not written -- the caller leaves its accumulator in place and comes back.  Not BOUNDED (request, redo):
// the caller cuts the buffer before a step could overflow it, and the kernel carries no compare (`cap` is not read).
template <bool BOUNDED>
__device__ __forceinline__ bool isim_append(uint64_t* cand, uint32_t* sh_cnt, uint32_t cap, bool want, uint64_t c) {
    const unsigned long long bal = __ballot(want);
    bool stored = false;
    if (bal) {
        const int lane = threadIdx.x & 63;
        uint32_t at = 0;
        if (lane == __ffsll((long long)bal) - 1) at = atomicAdd(sh_cnt, (uint32_t)__popcll(bal));
        at = __shfl(at, __ffsll((long long)bal) - 1, 64);
        if (want) {
            const uint32_t pos = at + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            if (!BOUNDED || pos < cap) { cand[pos] = c; stored = true; }
        }
    }
    return stored;
}

// The tail of a list: cut the *sh_cnt candidates to ~K (isim_select), pad to a power of two, sort.  Returns how many to keep; they
// are the front of cand, best first.  Every thread of the block calls it; the caller stores them its own way.
__device__ __forceinline__ int isim_finish_list(uint64_t* cand, int K, uint32_t* hist, uint32_t* sh_cnt, uint32_t* sh_tau, uint32_t* sh_aux) {
    isim_select(cand, (int)*sh_cnt, K, hist, sh_cnt, sh_tau, sh_aux);   // then only ~K entries are left to sort
    const int n = (int)*sh_cnt;
    int P2 = 1;
    while (P2 < n) P2 <<= 1;
    for (int i = n + threadIdx.x; i < P2; i += blockDim.x) cand[i] = 0ull;
    __syncthreads();
    fy_bitonic_desc(cand, P2);
    return min(n, K);
}

// one workgroup per row: fold the chunks' top-K lists (each sorted, disjoint columns) into the row's top K
__attribute__((unused)) static __global__ __launch_bounds__(256) void k_isim_merge(int32_t rows_mine, int32_t nch, int32_t K, const int32_t* __restrict__ part_cnt,
                                                    const uint64_t* __restrict__ part, int32_t* __restrict__ out_cnt,
                                                    int32_t* __restrict__ out_other, float* __restrict__ out_sim) {
    __shared__ uint64_t buf[2 * ISIM_MAX_K];
    const int tid = threadIdx.x;
    for (int m = blockIdx.x; m < rows_mine; m += gridDim.x) {
        int have = 0;
        for (int ch = 0; ch < nch; ch++) {
            const int n = part_cnt[(int64_t)m * nch + ch];
            if (n == 0) continue;    // block-uniform
            for (int i = tid; i < n; i += blockDim.x) buf[have + i] = part[((int64_t)m * nch + ch) * K + i];
            const int tot = have + n;
            if (have == 0) { have = n; __syncthreads(); continue; }   // a single list is already sorted
            int P2 = 1;
            while (P2 < tot) P2 <<= 1;
            for (int i = tot + tid; i < P2; i += blockDim.x) buf[i] = 0ull;
            __syncthreads();
            fy_bitonic_desc(buf, P2);
            have = min(tot, K);
        }
        __syncthreads();
        if (tid == 0) out_cnt[m] = have;
        for (int i = tid; i < have; i += blockDim.x) {
            const uint64_t c = buf[i];
            out_other[(int64_t)m * K + i] = isim_composite_item(c);
            out_sim[(int64_t)m * K + i] = isim_composite_sim_ordered(c);
        }
        __syncthreads();
    }
}

// the lists of rows -> the result, one wave per row.  rows: the popularity ranks of the rows (a request's, ascending); nullptr: the
// strided rows of a rank of the full build, rank + m * world
__attribute__((unused)) static __global__ void k_isim_compact(int32_t n, int32_t K, const int32_t* __restrict__ rows, int32_t rank, int32_t world,
                                                              const int32_t* __restrict__ cnt, const int32_t* __restrict__ off, const int32_t* __restrict__ other,
                                                              const float* __restrict__ sim, const int32_t* __restrict__ rank_item_raw, int32_t* __restrict__ o_item,
                                                              int32_t* __restrict__ o_other, float* __restrict__ o_sim, int32_t* __restrict__ o_aux) {
    const int wpb = blockDim.x >> 6, lane = threadIdx.x & 63;
    for (int32_t m = blockIdx.x * wpb + (threadIdx.x >> 6); m < n; m += gridDim.x * wpb) {
        const int32_t item = rank_item_raw[rows ? rows[m] : rank + m * world];
        for (int i = lane; i < cnt[m]; i += 64) {
            const int64_t o = (int64_t)off[m] + i;
            o_item[o] = item;
            o_other[o] = other[(int64_t)m * K + i];
            o_sim[o] = sim[(int64_t)m * K + i];
            o_aux[o] = 0;
        }
    }
}

}  // namespace fy
