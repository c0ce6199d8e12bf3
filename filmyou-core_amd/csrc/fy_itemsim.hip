// fy_itemsim.hip -- item-item similarity build (hot path #2): the co-rating row kernel with a top-K epilogue.
//
// Replaces Mahout 0.8's RowSimilarityJob as called at M/baselinerecommender/BaselineRecommenderJob.java:241-253
// (--similarityClassname, --maxSimilaritiesPerRow, --excludeSelfSimilarity, --threshold).  Parity is UNPINNED: the
// arithmetic is not in the reference tree and no reference test covers it; the algorithm
// restated here is Mahout's published one (see oracle/itemsim_oracle.c for the statement both sides implement):
//   cosine        sim(i, j) = sum_u (r_ui / |r_.i|) (r_uj / |r_.j|)      (rows L2-normalised, then dot products)
//   co-occurrence sim(i, j) = #users who rated both
// and the five other measures of Mahout 0.8's RowSimilarityJob (include/filmyou.h has the table): each is a dot product d of
// per-item transformed columns, then a scalar function of (d, a_i, a_j, number of users) -- the isim_finish_* functions of
// fy_itemsim_kernels.hpp, fp64, shared by every kernel that turns an accumulator into a similarity.  What a measure is (weight, norm,
// finish, kernel template) is the table isim_measure of fy_itemsim_plan.hpp; nothing here compares a measure id with a constant.
// Over co-rated pairs only, j != i when excludeSelfSimilarity, sim >= threshold (no threshold: sim > 0), the
// maxSimilaritiesPerRow best per item (ties, unspecified in Mahout, by ascending item id).
// Two builds; isim_route (fy_itemsim_plan.hpp, a pure host function with a CPU test) says which one a job takes:
//  * symmetric (round 3; cosine on positive fp16-exact ratings, one rank, the benchmark sizes): the product is symmetric, so
//    only its upper triangle is accumulated -- by the RM2 row kernel itself (fy_rm2.hip: gram_half_build: symmetric walk,
//    fixed-point ds_add_u64, half the pair visits) into an fp32 matrix in HBM -- and k_isim_sweep streams every element ONCE
//    for BOTH rows it belongs to: G[i][j] (i < j) is a candidate of row i where it is read along the row and of row j where
//    it is read down the column, 64 rows (= 256-byte row segments) at a time.  No mirror pass.
//  * row at a time (every other configuration): a workgroup owns item row i, accumulates it chunk by chunk in LDS (fp64) and
//    keeps a running top-K in LDS; no I x I matrix is written, only I x K rows leave the chip.
// Host flow of itemsim_build: isim_front (checks, input preparation, structure, norms -- shared with itemsim_prepare), the route,
// itemsim_symmetric or itemsim_row_at_a_time, k_isim_compact, statistics.  The prepared job of the request pass
// (fy_itemsim_request.hip) is built at the end of this file from the same front.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "fy_cooc.hpp"
#include "fy_itemsim_kernels.hpp"
#include "fy_itemsim_request.hpp"
#include "fy_prep.hpp"
#include "fy_rm2.hpp"

namespace fy {

// one WORKGROUP per item (pair): L2 norm of the item's rating column in a fixed summation order (thread-strided partial sums, wave
// shuffles, the four waves' partials in order), and -- round 4 -- the column's rating sum and largest rating in the same pass (the
// bounds of the fixed-point scale of the symmetric build; k_isim_gram_prep walked the columns a second time for them).  A wave per
// item made both passes wait for the heaviest column: 81 k entries on one wave = 1 270 dependent trips, 0.6 ms each pass.
// sumsq (optional): sum r^2 before the root (Euclidean distance).  PEARSON: a second walk of the column in the same fixed order
// for the centred norm -- centre[p] = (sum |r|) / n, cnorm[p] = || r - centre ||_2 over the item's raters; no atomics anywhere,
// two runs give the same bits.
template <bool PEARSON>
__global__ __launch_bounds__(256) void k_item_norms(int32_t nP, const int32_t* __restrict__ pair_start, const float* __restrict__ csc_r,
                                                    double* __restrict__ norm, float* __restrict__ colsum, float* __restrict__ colmax,
                                                    double* __restrict__ sumsq, double* __restrict__ centre, double* __restrict__ cnorm) {
    __shared__ double sh_s[4];
    __shared__ double sh_a[4], sh_centre;
    __shared__ float sh_sum[4], sh_max[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int32_t p = blockIdx.x; p < nP; p += gridDim.x) {
        double s = 0.0, sa = 0.0;
        float sum = 0.0f, mx = 0.0f;
        for (int32_t q = pair_start[p] + threadIdx.x; q < pair_start[p + 1]; q += 256) {
            const float r = csc_r[q];
            s += (double)r * (double)r;
            sum += r;
            mx = fmaxf(mx, r);
            if constexpr (PEARSON) sa += fabs((double)r);
        }
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_down(s, o, 64);
            sum += __shfl_down(sum, o, 64);
            mx = fmaxf(mx, __shfl_down(mx, o, 64));
            if constexpr (PEARSON) sa += __shfl_down(sa, o, 64);
        }
        if (lane == 0) { sh_s[wave] = s; sh_sum[wave] = sum; sh_max[wave] = mx; if constexpr (PEARSON) sh_a[wave] = sa; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const double ss = ((sh_s[0] + sh_s[1]) + sh_s[2]) + sh_s[3];
            norm[p] = sqrt(ss);
            if (sumsq) sumsq[p] = ss;
            if (colsum) colsum[p] = ((sh_sum[0] + sh_sum[1]) + sh_sum[2]) + sh_sum[3];
            if (colmax) colmax[p] = fmaxf(fmaxf(sh_max[0], sh_max[1]), fmaxf(sh_max[2], sh_max[3]));
            if constexpr (PEARSON) sh_centre = (((sh_a[0] + sh_a[1]) + sh_a[2]) + sh_a[3]) / (double)(pair_start[p + 1] - pair_start[p]);
        }
        __syncthreads();
        if constexpr (PEARSON) {
            const double c = sh_centre;
            double s2 = 0.0;
            for (int32_t q = pair_start[p] + threadIdx.x; q < pair_start[p + 1]; q += 256) {
                const double x = (double)csc_r[q] - c;
                s2 += x * x;
            }
            for (int o = 32; o > 0; o >>= 1) s2 += __shfl_down(s2, o, 64);
            __syncthreads();      // everybody has read sh_centre; sh_s is free again
            if (lane == 0) sh_s[wave] = s2;
            __syncthreads();
            if (threadIdx.x == 0) {
                centre[p] = c;
                cnorm[p] = sqrt(((sh_s[0] + sh_s[1]) + sh_s[2]) + sh_s[3]);
            }
            __syncthreads();
        }
    }
}

// ---- the weight of a preference (fy_itemsim_plan.hpp: IsimMeasure) where nothing is applied in the epilogue: the 8-byte walk.
// norm: cosine ||r_.i||, Pearson ||c_.i||; centre: Pearson (sum |r|) / n (else unused)
__device__ __forceinline__ float isim_weight(const IsimMeasure& m, float r, double norm, double centre) {
    switch (m.weight) {
        case ISIM_W_RATING: return m.inv_norm ? (float)((double)r / norm) : r;
        case ISIM_W_PEARSON: return (float)(((double)r - centre) / norm);       // 0 / 0 = NaN for a constant item: its pairs drop out
        default: return 1.0f;
    }
}
__global__ void k_csc_weights(int64_t nnz, const int32_t* __restrict__ csc_pair, const float* __restrict__ csc_r,
                              const double* __restrict__ norm, const double* __restrict__ centre, int measure, float* __restrict__ csc_w) {
    const IsimMeasure m = isim_measure(measure);
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * blockDim.x) {
        const int32_t p = csc_pair[q];
        csc_w[q] = isim_weight(m, csc_r[q], norm[p], m.weight == ISIM_W_PEARSON ? centre[p] : 0.0);
    }
}

__global__ void k_csr_weights(int64_t nnz, const int32_t* __restrict__ csr_idx, const float* __restrict__ csr_r,
                              const int32_t* __restrict__ rank_pair, const double* __restrict__ norm, const double* __restrict__ centre, int measure,
                              float* __restrict__ csr_w) {
    const IsimMeasure m = isim_measure(measure);
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < nnz; f += (int64_t)gridDim.x * blockDim.x) {
        const int32_t p = rank_pair[csr_idx[f]];
        csr_w[f] = isim_weight(m, csr_r[f], norm[p], m.weight == ISIM_W_PEARSON ? centre[p] : 0.0);
    }
}

// dynamic LDS: [CH doubles accumulators][ISIM_CAP uint64 candidates].  Persistent workgroups pull (row, column chunk) ITEMS
// from a global counter (heavy rows first) and leave the top K of that chunk; k_isim_merge folds a row's chunks together.
// Only the heaviest rows are split by chunk (one workgroup per whole row left the heaviest row -- 10^5 raters, 5e7 slice
// entries -- on a single CU for half of the kernel's run time); a light row is one item and carries its threshold from chunk
// to chunk (splitting every row cost more in top-K work than it gained: 52 ms against 30).  The pass that streams a finished chunk through the top-K re-zeroes the accumulators it reads.
template <bool PK, int M>
__global__ void k_cooc_itemsim(CoocArgs A, ISimEpilogue E, int* __restrict__ next_row) {
    double* acc = fy_cooc_acc;
    uint64_t* cand = reinterpret_cast<uint64_t*>(fy_cooc_acc + A.CH);
    __shared__ uint32_t sh_cnt, sh_tau, sh_aux[2], hist[256];
    __shared__ int sh_row;
    const int tid = threadIdx.x;
    const int stride = A.row_stride ? A.row_stride : 1;
    for (int t = tid; t < A.CH; t += blockDim.x) acc[t] = 0.0;
    int next = 0;
    if (tid == 0) next = atomicAdd(next_row, 1);
    for (;;) {
        if (tid == 0) { sh_row = next; sh_cnt = 0; sh_tau = 0; }
        __syncthreads();
        const int item = sh_row;
        if (item >= E.n_items) break;
        if (tid == 0) next = atomicAdd(next_row, 1);   // the round trip hides behind this item's work
        // the first heavy_rows rows are split into one item per column chunk, every other row is one item
        const bool split = item < E.heavy_rows * A.nch;
        const int mine = split ? item / A.nch : E.heavy_rows + (item - E.heavy_rows * A.nch);
        const int ch_begin = split ? item - mine * A.nch : 0, ch_end = split ? ch_begin + 1 : A.nch;
        const int slot = mine * A.nch + ch_begin;     // where this item's list goes
        const int row = A.row0 + mine * stride;
        const double scale_row = isim_row_scale<M>(E, row);
        for (int ch = ch_begin; ch < ch_end; ch++) {
            cooc_accumulate_row<PK>(A, row, ch, mine);
            __syncthreads();
            const int c0 = ch * A.CH;
            const int ncol = min(A.CH, A.Ic - c0);
            // Stream the finished chunk through the running top-K: values >= tau are appended to the candidate buffer, every
            // accumulator that has been looked at is re-zeroed.  The whole chunk is taken WITHOUT a barrier (one barrier per
            // 1024 columns was a third of the kernel); a candidate that finds the buffer full leaves its accumulator in place,
            // the buffer is cut back (isim_select raises tau) and the pass runs again over what is left.  A consumed entry
            // reads as similarity 0, which only a threshold <= 0 would accept again: that configuration steps with barriers.
            const bool stepwise = E.has_threshold && !(E.threshold > 0.0f);
            if (!stepwise && sh_tau == 0 && ncol >= 4 * ISIM_SAMPLE) {
                // No threshold yet: thousands of non-zero similarities would flood the candidate buffer and be cut back in
                // several rounds.  Guess one from a sample instead: the ISIM_SAMPLE_RANK-th largest of ISIM_SAMPLE columns
                // spread over the chunk (wave 0, shuffles only), count how many columns reach it (one sweep, no writes) and
                // adopt it if at least K do -- then it is a valid lower bound of the K-th best and the append pass below
                // takes a few hundred candidates in one go.  A bad guess changes nothing: the old path runs.
                if (tid < 64) {
                    uint32_t k4[ISIM_SAMPLE / 64];
#pragma unroll
                    for (int x = 0; x < ISIM_SAMPLE / 64; x++) {
                        const int t = (int)(((int64_t)(tid * (ISIM_SAMPLE / 64) + x) * ncol) / ISIM_SAMPLE);
                        uint32_t key;
                        const bool ok = isim_candidate<M>(E, acc[t], scale_row, row, c0 + t, key);
                        k4[x] = ok ? key : 0u;
                    }
                    uint32_t best = 0;
                    for (int r = 0; r < ISIM_SAMPLE_RANK; r++) {
                        uint32_t m = 0;
#pragma unroll
                        for (int x = 0; x < ISIM_SAMPLE / 64; x++) m = max(m, k4[x]);
                        uint32_t wm = m;
                        for (int o = 32; o > 0; o >>= 1) wm = max(wm, (uint32_t)__shfl_xor((int)wm, o, 64));
                        best = wm;
                        // remove one occurrence of the maximum (the first lane that holds it)
                        const unsigned long long holders = __ballot(m == wm && wm != 0);
                        if (holders && tid == __ffsll((long long)holders) - 1) {
                            bool done = false;
#pragma unroll
                            for (int x = 0; x < ISIM_SAMPLE / 64; x++)
                                if (!done && k4[x] == wm) { k4[x] = 0; done = true; }
                        }
                    }
                    if (tid == 0) { sh_aux[0] = best; sh_aux[1] = 0; }
                }
                __syncthreads();
                const uint32_t guess = sh_aux[0];
                if (guess != 0) {   // block-uniform
                    int mine_cnt = 0;
                    for (int t = tid; t < ncol; t += blockDim.x) {
                        uint32_t key;
                        const bool ok = isim_candidate<M>(E, acc[t], scale_row, row, c0 + t, key);
                        mine_cnt += ok && key >= guess;
                    }
                    for (int o = 32; o > 0; o >>= 1) mine_cnt += __shfl_down(mine_cnt, o, 64);
                    if ((tid & 63) == 0 && mine_cnt) atomicAdd(&sh_aux[1], (uint32_t)mine_cnt);
                    __syncthreads();
                    if (tid == 0 && sh_aux[1] >= (uint32_t)E.K) sh_tau = guess;
                }
                __syncthreads();
            }
            for (bool again = true; again;) {
                const uint32_t tau = sh_tau;
                for (int base = 0; base < ncol; base += blockDim.x) {
                    const int t = base + tid;
                    bool want = false;
                    uint64_t c = 0;
                    if (t < ncol) {
                        const int col = c0 + t;
                        uint32_t key;
                        const bool ok = isim_candidate<M>(E, acc[t], scale_row, row, col, key);
                        want = ok && key >= (stepwise ? sh_tau : tau);
                        if (want) c = isim_composite(key, E.rank_item_raw[col]);
                        else acc[t] = 0.0;
                    }
                    if (isim_append<true>(cand, &sh_cnt, (uint32_t)E.cap, want, c)) acc[t] = 0.0;
                    if (stepwise) {
                        __syncthreads();
                        if (sh_cnt + blockDim.x > (uint32_t)E.cap) isim_cut(cand, E.K, E.cap, hist, &sh_cnt, &sh_tau, sh_aux);
                    }
                }
                __syncthreads();
                again = false;
                if (!stepwise && sh_cnt > (uint32_t)E.cap) {   // block-uniform: some candidates did not fit
                    __syncthreads();
                    if (tid == 0) sh_cnt = (uint32_t)E.cap;
                    __syncthreads();
                    isim_cut(cand, E.K, E.cap, hist, &sh_cnt, &sh_tau, sh_aux);
                    again = true;
                }
            }
        }
        const int keep = isim_finish_list(cand, E.K, hist, &sh_cnt, &sh_tau, sh_aux);
        if (tid == 0) E.part_cnt[slot] = keep;
        for (int i = tid; i < keep; i += blockDim.x) E.part[(int64_t)slot * E.K + i] = cand[i];
        __syncthreads();   // everybody is done with sh_cnt / cand before the next item resets them
    }
}


// ================================================================ symmetric build: band sweep over the fp32 half Gram
// G (fy_rm2.hip: gram_half_build): row i holds sum_v r_vi r_vj for the columns j > i (exact zeros for (i & ~255) <= j <= i,
// nothing in front).  sim(i, j) = G * inv_norm[i] * inv_norm[j].  A workgroup owns a PIECE = (band of 64 rows [i0, i0 + 64)) x
// (column range [c0, c1)):
//   * "down the column": for every row j in [c0, c1) above the band (j < i0 + lane), the 256-byte segment G[j][i0 .. i0 + 64) --
//     lane l looks at the candidate j of ITS row i0 + l;
//   * "along the row": for every row of the band, G[i][max(c0, i0) .. c1) in 1 KB tiles -- all lanes look at candidates of one row.
// Every element of the triangle is read exactly once by each of the two rows it belongs to; a band's pieces have equal size.
// Running top-K without a sort: a candidate must reach the row's threshold key tau (float bits order like the floats: all
// similarities here are > 0).  Passing candidates are appended to the row's list in HBM and counted in the row's 64-bucket
// histogram of their keys (8 buckets per octave below 1.0; in HBM / L2, shared by the band's pieces); every 8th candidate of a
// row that has K, tau rises to the lower edge of the highest bucket with K candidates at or above it -- a valid lower bound of
// the row's final K-th best (they are K real candidates of the row), published to the band's other pieces through tau_g.  After warm-up a few candidates per thousand
// pass; k_isim_finish selects and sorts the lists.  A row whose list overflows (massive ties inside one bucket) is redone
// exactly by k_isim_finish from the matrix.
constexpr int SWEEP_KEY_SHIFT = 20, SWEEP_KEY_BASE = 1016 - 63;   // bucket = (key >> 20) - base: 63 <-> [1, 1.125), 0 <-> everything below 2^-7.875
struct SweepArgs {
    const float* __restrict__ G;
    int64_t ldm;
    int32_t Ic, K;
    // cosine: 1 / norm in rank order; the finishing measures (Tanimoto, log-likelihood, city block, Euclidean distance): a_i
    const float* __restrict__ invn32;          // [ldm + slack] fp32 (0 behind Ic): the prefilter
    const double* __restrict__ invn;           // [Ic]
    double n_cols;                             // N (log-likelihood)
    const int32_t* __restrict__ rank_item_raw;
    uint32_t* __restrict__ tau_g;              // [Ic]: key a candidate of the row must reach
    int32_t* __restrict__ gcnt;                // [Ic]: candidates appended
    uint64_t* __restrict__ glist;              // [Ic][capg]: isim_composite of the positive key
    int32_t capg;
    int32_t* __restrict__ overflow;            // [Ic]
    uint32_t* __restrict__ hist_g;             // [Ic][64]: the row's candidates by key bucket (all pieces of the band add to it)
    int32_t nbands, piece;
    uint32_t tau0;                             // the job's own threshold as a key (1 = "similarity > 0")
    int32_t exclude_self;
    int32_t* __restrict__ out_cnt;             // k_isim_finish: [Ic], [Ic * K], [Ic * K]
    int32_t* __restrict__ out_other;
    float* __restrict__ out_sim;
};

// The symmetric build per measure M (FY_SIMILARITY_COSINE: similarity = G x a per-row factor x a per-column factor, the code this
// build was written for).  sweep_pre: the fp32 value the fast path compares with the row's threshold (with its margin).  Tanimoto
// and city block are one or two roundings of exact integers (counts below 2^24), so the margin holds for them as it does for
// cosine; log-likelihood (cancelling x ln x terms) and Euclidean distance (a_i - 2 d + a_j cancels) have no fp32 value with a
// relative bound: every co-rated element passes the prefilter (+inf) and is decided in fp64 by sweep_value.  An element nobody
// co-rated (G == 0) is never a candidate.
template <int M>
__device__ __forceinline__ float sweep_pre(float v, float a, float b) {
    if constexpr (M == FY_SIMILARITY_COSINE) return v * a * b;
    else if constexpr (M == FY_SIMILARITY_TANIMOTO_COEFFICIENT) return v != 0.0f ? v / (a + b - v) : 0.0f;
    else if constexpr (M == FY_SIMILARITY_CITY_BLOCK) return v != 0.0f ? 1.0f / (1.0f + a + b - 2.0f * v) : 0.0f;
    else return v != 0.0f ? __builtin_inff() : 0.0f;
}
template <int M>
__device__ __forceinline__ float sweep_value(const SweepArgs& A, float v, int i, int col) {
    if constexpr (M == FY_SIMILARITY_COSINE) return (float)isim_finish_product((double)v, A.invn[i], A.invn[col]);
    else return v != 0.0f ? (float)isim_finish<M>((double)v, A.invn[i], A.invn[col], A.n_cols) : 0.0f;
}

// wave-level: lanes with `pass` hold a candidate (row i = band row rl, column col, raw Gram value v) that survived the fp32
// prefilter; exact value, append, histogram, and -- every 8th candidate of a row once it has K -- a new threshold for the row
template <int M>
__device__ __forceinline__ void sweep_take(const SweepArgs& A, uint32_t* tau_l, bool pass, int rl, int i, int col, float v, int i0) {
    const int lane = threadIdx.x & 63;
    bool trig = false;
    if (pass) {
        const float sf = sweep_value<M>(A, v, i, col);
        const uint32_t key = isim_positive_key(sf);
        if (sf > 0.0f && key >= tau_l[rl]) {
            int bk = (int)(key >> SWEEP_KEY_SHIFT) - SWEEP_KEY_BASE;
            bk = bk < 0 ? 0 : (bk > 63 ? 63 : bk);
            atomicAdd(&A.hist_g[(int64_t)i * 64 + bk], 1u);
            const int pos = atomicAdd(&A.gcnt[i], 1);
            if (pos < A.capg) A.glist[(int64_t)i * A.capg + pos] = isim_composite(key, A.rank_item_raw[col]);
            else A.overflow[i] = 1;
            trig = pos + 1 >= A.K && ((pos + 1) & 7) == 0;
        }
    }
    unsigned long long m = __ballot(trig);
    while (m) {   // wave-uniform
        const int src = __ffsll((long long)m) - 1;
        const int r = __shfl(rl, src, 64);
        m &= ~__ballot(rl == r);                       // (along a row every lane holds the same row)
        // suffix sums over the row's buckets: candidates at or above bucket `lane`, over ALL pieces of the band (the histogram
        // is the row's, in HBM / L2: the first version kept one per piece in LDS, and a piece sees a seventh of the row -- its K-th
        // best is the row's 7 K-th: 1157 candidates per row for K = 100)
        uint32_t h = A.hist_g[(int64_t)(i0 + r) * 64 + lane];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_down((int)h, o, 64);
            if (lane + o < 64) h += t;
        }
        const unsigned long long ok = __ballot(h >= (uint32_t)A.K);
        if (ok) {
            const int B = 63 - __clzll((long long)ok);
            if (B > 0 && lane == 0) {
                const uint32_t nt = (uint32_t)(B + SWEEP_KEY_BASE) << SWEEP_KEY_SHIFT;
                atomicMax(&tau_l[r], nt);
                atomicMax(&A.tau_g[i0 + r], nt);
            }
        }
    }
}

template <int M>
__global__ __launch_bounds__(256) void k_isim_sweep(SweepArgs A) {
    extern __shared__ __attribute__((aligned(16))) float fy_sweep_lds[];      // [piece + 256]: 1 / norm of the piece's columns, then 64: of the band's rows
    __shared__ uint32_t tau_l[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p = blockIdx.x / A.nbands, b = blockIdx.x - p * A.nbands;
    const int i0 = b * 64;
    const int c0 = p * A.piece, c1 = min(c0 + A.piece, (int)A.ldm);
    float* __restrict__ nrm_cols = fy_sweep_lds;
    float* __restrict__ nrm_rows = fy_sweep_lds + A.piece + 256;
    // the norms the piece needs, once: every element used to bring its column's norm along from L2 (a second 16-byte load per
    // 16 bytes of the matrix), and every row of the band began with a dependent load of its own norm
    for (int t = tid; t < A.piece + 256; t += 256) nrm_cols[t] = c0 + t < (int)A.ldm ? A.invn32[c0 + t] : 0.0f;
    if (tid < 64) {
        nrm_rows[tid] = A.invn32[i0 + tid];
        tau_l[tid] = i0 + tid < A.Ic ? A.tau_g[i0 + tid] : 0xFFFFFFFFu;
    }
    __syncthreads();
    // The fast path of both parts is straight-line: U loads in flight, one compare per element against the row's threshold in
    // fp32 with a margin, the outcome kept as one bit per element.  Only when some lane of the wave holds a set bit does the
    // wave enter the slow path -- ONE copy of sweep_take per part, each lane presenting its own lowest set element.  (The first
    // version called sweep_take from every unrolled compare: 24 inlined copies, and it read the column-side norms with
    // wave-uniform loads that the compiler turned into dependent vector loads behind s_waitcnt vmcnt(0): 8.6 ms for 14 GB.)
    // ---- down the column: rows j of the matrix in [c0, jend), segment [i0, i0 + 64); wave w takes j = c0 + w, c0 + w + 4, ...
    const int jend = min(min(c1, i0 + 64), A.Ic);
    if (c0 < jend && A.exclude_self != 3) {
        const int i = i0 + lane;
        const bool valid = i < A.Ic;
        const float my_inv = valid ? nrm_rows[lane] : 0.0f;
        const float* __restrict__ gp = A.G + i0 + lane;
        constexpr int U = 8;
        for (int jb = c0 + wave; jb < jend; jb += 4 * 64) {     // 64 of the wave's rows per block: their norms in one read, lane k <-> row jb + 4 k
            const float nj_vec = nrm_cols[min(jb + 4 * lane, jend - 1) - c0];
            for (int k0 = 0; k0 < 64 && jb + 4 * k0 < jend; k0 += U) {     // wave-uniform
                float v[U];
#pragma unroll
                for (int u = 0; u < U; u++) v[u] = gp[(int64_t)min(jb + 4 * (k0 + u), jend - 1) * A.ldm];     // unconditional loads (a clamped row is masked below)
                const float tauf = __uint_as_float(tau_l[lane]) * 0.999999f;
                uint32_t pm = 0;
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int jj = jb + 4 * (k0 + u);
                    const float nj = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(nj_vec), k0 + u));
                    const float s = sweep_pre<M>(v[u], nj, my_inv);
                    // (bitwise, not &&: short-circuit evaluation turned these into exec-masked branches around the loads)
                    pm |= ((uint32_t)valid & (uint32_t)(jj < jend) & (uint32_t)(jj < i) & (uint32_t)(s > 0.0f) & (uint32_t)(s >= tauf)) << u;
                }
                while (__ballot(pm != 0)) {      // slow path: rare once the thresholds have warmed up
                    const int u = pm ? __ffs((int)pm) - 1 : 0;
                    float vu = v[0];
#pragma unroll
                    for (int q = 1; q < U; q++) vu = u == q ? v[q] : vu;
                    sweep_take<M>(A, tau_l, pm != 0, lane, i, jb + 4 * (k0 + u), vu, i0);
                    pm &= pm - 1;
                }
            }
        }
    }
    // ---- along the row: columns [cs, c1) of the band's rows (a row's candidates are the columns behind it).  ONE loop over the
    // (row, 256-column tile) pairs of this wave -- rows wave, wave + 4, ... -- four tiles in flight, also across the end of a row
    const int cs = max(c0, i0);
    const int n_rows = min(64, A.Ic - i0);
    if (cs < c1 && wave < n_rows && A.exclude_self != 2) {
        constexpr int U = 4;
        const int tiles_per_row = (c1 - cs + 255) >> 8;
        const int total = ((n_rows - wave + 3) >> 2) * tiles_per_row;
        int rr = wave, tt = 0;                                  // row / tile of pair T0 (wave-uniform)
        for (int T0 = 0; T0 < total; T0 += U) {
            float4 v[U];
            int r_of[U], col_of[U];
            {
                int r2 = rr, t2 = tt;
#pragma unroll
                for (int u = 0; u < U; u++) {
                    r_of[u] = r2;
                    col_of[u] = cs + 256 * t2 + 4 * lane;      // (a tile that overshoots c1 reads the slack behind the row / the matrix: masked below)
                    v[u] = *reinterpret_cast<const float4*>(A.G + (int64_t)(i0 + r2) * A.ldm + col_of[u]);
                    if (T0 + u + 1 < total) { if (++t2 == tiles_per_row) { t2 = 0; r2 += 4; } }     // (the last pairs repeat: masked by T0 + u < total)
                }
                rr = r2; tt = t2;                             // = pair T0 + U
            }
            float vv[4 * U];
            uint32_t pm = 0;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int i = i0 + r_of[u];
                const float ri = nrm_rows[r_of[u]];
                const float tauf = __uint_as_float(tau_l[r_of[u]]) * 0.999999f;
                const float4 n4 = *reinterpret_cast<const float4*>(nrm_cols + (col_of[u] - c0));
                vv[4 * u + 0] = v[u].x; vv[4 * u + 1] = v[u].y; vv[4 * u + 2] = v[u].z; vv[4 * u + 3] = v[u].w;
                const float nn[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int col = col_of[u] + e;
                    const float s = sweep_pre<M>(vv[4 * u + e], ri, nn[e]);
                    pm |= ((uint32_t)(T0 + u < total) & (uint32_t)(col < c1) & (uint32_t)(col > i) & (uint32_t)(col < A.Ic) & (uint32_t)(s > 0.0f) & (uint32_t)(s >= tauf)) << (4 * u + e);
                }
            }
            while (__ballot(pm != 0)) {
                const int x = pm ? __ffs((int)pm) - 1 : 0;
                float vx = vv[0];
#pragma unroll
                for (int q = 1; q < 4 * U; q++) vx = x == q ? vv[q] : vx;
                int rx = r_of[0], cx = col_of[0];
#pragma unroll
                for (int q = 1; q < U; q++) { rx = (x >> 2) == q ? r_of[q] : rx; cx = (x >> 2) == q ? col_of[q] : cx; }
                sweep_take<M>(A, tau_l, pm != 0, rx, i0 + rx, cx + (x & 3), vx, i0);
                pm &= pm - 1;
            }
        }
    }
}

// (LDS traffic between the lanes of ONE wave needs no s_barrier -- a wave's LDS instructions complete in order -- only a
// compiler fence, so that a lane's read of another lane's word is not moved in front of the writes)
__device__ __forceinline__ void isim_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// the diagonal candidate of row i (not part of the triangle): sum r^2 / norm^2; 0 = none
template <int M>
__device__ __forceinline__ uint64_t isim_self_candidate(const SweepArgs& A, int i) {
    if (A.exclude_self) return 0ull;
    float sf;
    if constexpr (M == FY_SIMILARITY_COSINE) {
        const double inv_i = A.invn[i], nrm = 1.0 / inv_i;
        sf = (float)(nrm * nrm * inv_i * inv_i);
    } else {
        const double a = A.invn[i];      // the item's dot product with itself is its own norm (number of raters; sum r^2)
        sf = (float)isim_finish<M>(a, a, a, A.n_cols);
    }
    const uint32_t key = isim_positive_key(sf);
    return (sf > 0.0f && key >= A.tau0) ? isim_composite(key, A.rank_item_raw[i]) : 0ull;
}

// One WAVE per row: the K best of the row's candidate list (a few hundred entries of 8 bytes, L2-resident), sorted by
// descending similarity, ties by ascending item id -- the order of the composite key << 32 | (0x7FFFFFFF - id), all distinct.
// More than FIN_SMALL candidates are first cut by a radix select over the composite, 8 bits per level from the top, until the
// entries at or above the prefix fit the sort buffer (two levels = 16 key bits in practice; eight levels are exact for any
// input).  No workgroup barrier anywhere: 59 047 workgroups with ~40 barriers each were 2.0 ms, this is one pass of waves.
// Rows whose list overflowed in the sweep are handed to k_isim_redo.
constexpr int FIN_SURV = 512, FIN_SMALL = 128;
static_assert(FIN_SURV == ISIM_PLAN_FIN_SURV, "fy_itemsim_plan.hpp routes by the list length k_isim_finish can sort");
template <int M>
__global__ __launch_bounds__(256) void k_isim_finish(SweepArgs A, int32_t* __restrict__ redo_list, int32_t* __restrict__ n_redo) {
    __shared__ uint64_t surv_all[4][FIN_SURV];
    __shared__ uint32_t hist_all[4][256];
    __shared__ uint32_t scal_all[4][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + w;
    if (i >= A.Ic) return;                               // wave-uniform; nothing below synchronises the workgroup
    if (A.overflow[i]) {
        if (lane == 0) redo_list[atomicAdd(n_redo, 1)] = i;
        return;
    }
    uint64_t* surv = surv_all[w];
    uint32_t* hist = hist_all[w];
    uint32_t* scal = scal_all[w];
    const int n = min(A.gcnt[i], A.capg);
    const uint64_t* __restrict__ L = A.glist + (int64_t)i * A.capg;
    const uint64_t c_self = isim_self_candidate<M>(A, i);
    const int m = n + (c_self ? 1 : 0);
    auto get = [&](int t) -> uint64_t { return t < n ? L[t] : c_self; };
    int cnt = 0;
    if (m <= FIN_SMALL || m <= A.K) {                   // (K <= 512 = FIN_SURV here: itemsim_symmetric)
        for (int t = lane; t < m && t < FIN_SURV; t += 64) surv[t] = get(t);
        cnt = min(m, FIN_SURV);
        if (m > FIN_SURV) cnt = -1;                      // K > FIN_SURV never reaches this kernel
    } else {
        uint64_t prefix = 0;
        uint32_t above = 0;
        int shift = 56;
        for (;; shift -= 8) {
            for (int bb = lane; bb < 256; bb += 64) hist[bb] = 0u;
            isim_wave_sync();
            const uint64_t hi_mask = shift == 56 ? 0ull : ~0ull << (shift + 8);
            for (int t = lane; t < m; t += 64) {
                const uint64_t c = get(t);
                if ((c & hi_mask) == prefix) atomicAdd(&hist[(uint32_t)(c >> shift) & 255u], 1u);
            }
            isim_wave_sync();
            if (lane == 0) {
                uint32_t cum = above;
                int bb = 255;
                for (; bb > 0; bb--) {
                    if (cum + hist[bb] >= (uint32_t)A.K) break;
                    cum += hist[bb];
                }
                scal[0] = (uint32_t)bb;
                scal[1] = cum;
                scal[2] = cum + hist[bb];
            }
            isim_wave_sync();
            prefix |= (uint64_t)scal[0] << shift;
            above = scal[1];
            const uint32_t at_or_above = scal[2];
            isim_wave_sync();
            if (at_or_above <= (uint32_t)FIN_SURV || shift == 0) break;      // (shift == 0: the prefix is the K-th composite itself)
        }
        if (lane == 0) scal[3] = 0u;
        isim_wave_sync();
        for (int t0 = 0; t0 < m; t0 += 64) {
            const int t = t0 + lane;
            const uint64_t c = t < m ? get(t) : 0ull;
            const bool keep = t < m && c >= prefix;
            const unsigned long long bal = __ballot(keep);
            if (bal) {
                const uint32_t base = scal[3];
                if (keep) {
                    const uint32_t pos = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                    if (pos < (uint32_t)FIN_SURV) surv[pos] = c;
                }
                isim_wave_sync();
                if (lane == 0) scal[3] = base + (uint32_t)__popcll(bal);
                isim_wave_sync();
            }
        }
        cnt = (int)min(scal[3], (uint32_t)FIN_SURV);
    }
    int P2 = 1;
    while (P2 < cnt) P2 <<= 1;
    for (int t = cnt + lane; t < P2; t += 64) surv[t] = 0ull;
    isim_wave_sync();
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < P2; t += 64) {
                const int l = t ^ j;
                if (l > t) {
                    const uint64_t x = surv[t], y = surv[l];
                    const bool desc = (t & k) == 0;
                    if (desc ? (x < y) : (x > y)) { surv[t] = y; surv[l] = x; }
                }
            }
            isim_wave_sync();
        }
    const int keep = min(cnt, A.K);
    if (lane == 0) A.out_cnt[i] = keep;
    for (int t = lane; t < keep; t += 64) {
        const uint64_t c = surv[t];
        A.out_other[(int64_t)i * A.K + t] = isim_composite_item(c);
        A.out_sim[(int64_t)i * A.K + t] = isim_composite_sim_positive(c);
    }
}

// rows whose candidate list overflowed (massive ties inside one bucket of the sweep's histogram): every column of the row, from
// the matrix, through the running top-K of the row-at-a-time kernel (isim_cut: exact for any input)
template <int M>
__global__ __launch_bounds__(256) void k_isim_redo(SweepArgs A, const int32_t* __restrict__ redo_list, const int32_t* __restrict__ n_redo) {
    __shared__ uint64_t cand[ISIM_CAP];
    __shared__ uint32_t sh_cnt, sh_tau, sh_aux[2], hist[256];
    const int tid = threadIdx.x;
    const int n_rows = *n_redo;
    for (int x = blockIdx.x; x < n_rows; x += gridDim.x) {      // block-uniform
        const int i = redo_list[x];
        if (tid == 0) { sh_cnt = 0; sh_tau = A.tau0; }
        __syncthreads();
        for (int base = 0; base < A.Ic; base += 256) {
            const int col = base + tid;
            bool want = false;
            uint64_t c = 0;
            if (col < A.Ic && col != i) {
                const float v = col > i ? A.G[(int64_t)i * A.ldm + col] : A.G[(int64_t)col * A.ldm + i];
                const float sf = sweep_value<M>(A, v, i, col);
                const uint32_t key = isim_positive_key(sf);
                want = sf > 0.0f && key >= sh_tau;
                c = isim_composite(key, A.rank_item_raw[col]);
            }
            isim_append<false>(cand, &sh_cnt, 0, want, c);
            __syncthreads();
            if (sh_cnt + 256 + 1 > (uint32_t)ISIM_CAP) isim_cut(cand, A.K, ISIM_CAP, hist, &sh_cnt, &sh_tau, sh_aux);   // block-uniform (+ 1: the diagonal)
        }
        const uint64_t c_self = isim_self_candidate<M>(A, i);
        if (c_self && tid == 0) cand[sh_cnt++] = c_self;
        __syncthreads();
        const int keep = isim_finish_list(cand, A.K, hist, &sh_cnt, &sh_tau, sh_aux);
        if (tid == 0) A.out_cnt[i] = keep;
        for (int t = tid; t < keep; t += 256) {
            const uint64_t c = cand[t];
            A.out_other[(int64_t)i * A.K + t] = isim_composite_item(c);
            A.out_sim[(int64_t)i * A.K + t] = isim_composite_sim_positive(c);
        }
        __syncthreads();     // everybody is done with cand / sh_cnt before the next row resets them
    }
}
__global__ void k_sum_i32(int32_t n, const int32_t* __restrict__ v, unsigned long long* __restrict__ out) {
    unsigned long long s = 0;
    for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) s += (unsigned long long)v[t];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

// per item in rank order: 1 / norm (fp64 and fp32) and the bounds of the fixed-point scale (largest column sum / largest rating, from
// k_item_norms' per-column sums and maxima: no second walk over the columns)
__global__ void k_isim_gram_prep(int32_t Ic, int64_t ld_pad, const int32_t* __restrict__ rank_pair, const float* __restrict__ colsum,
                                 const float* __restrict__ colmax, const double* __restrict__ norm, double* __restrict__ invn, float* __restrict__ invn32,
                                 uint32_t* __restrict__ bounds /* [0] max column sum, [1] max rating, as float bits */) {
    float bs = 0.0f, bm = 0.0f;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < ld_pad; r += (int64_t)gridDim.x * blockDim.x) {
        if (r >= Ic) { invn32[r] = 0.0f; continue; }
        const int32_t pr = rank_pair[r];
        const double inv = 1.0 / norm[pr];
        invn[r] = inv;
        invn32[r] = (float)inv;
        bs = fmaxf(bs, colsum[pr] * 1.0001f);
        bm = fmaxf(bm, colmax[pr]);
    }
    // positive floats order like their bits; one atomic per wave (59 047 atomics on ONE address took 1.4 ms: 82 M/s)
    for (int o = 32; o > 0; o >>= 1) { bs = fmaxf(bs, __shfl_down(bs, o, 64)); bm = fmaxf(bm, __shfl_down(bm, o, 64)); }
    if ((threadIdx.x & 63) == 0) {
        if (__float_as_uint(bs) > bounds[0]) atomicMax(&bounds[0], __float_as_uint(bs));
        if (__float_as_uint(bm) > bounds[1]) atomicMax(&bounds[1], __float_as_uint(bm));
    }
}
// the same for the finishing measures: a_i (rank order, fp64: k_isim_rank_norms) as fp32 for the prefilter, and the bounds of the
// fixed-point scale -- the count measures multiply ones (largest column sum = largest n_i, largest value 1), Euclidean distance
// the ratings (cosine's bounds)
__global__ void k_isim_gram_prep_aux(int32_t Ic, int64_t ld_pad, const int32_t* __restrict__ rank_pair, const float* __restrict__ colsum,
                                     const float* __restrict__ colmax, const double* __restrict__ aux, int counts, float* __restrict__ a32,
                                     uint32_t* __restrict__ bounds) {
    float bs = 0.0f, bm = 0.0f;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < ld_pad; r += (int64_t)gridDim.x * blockDim.x) {
        if (r >= Ic) { a32[r] = 0.0f; continue; }
        a32[r] = (float)aux[r];
        const int32_t pr = rank_pair[r];
        bs = fmaxf(bs, (counts ? (float)aux[r] : colsum[pr]) * 1.0001f);
        bm = fmaxf(bm, counts ? 1.0f : colmax[pr]);
    }
    for (int o = 32; o > 0; o >>= 1) { bs = fmaxf(bs, __shfl_down(bs, o, 64)); bm = fmaxf(bm, __shfl_down(bm, o, 64)); }
    if ((threadIdx.x & 63) == 0) {
        if (__float_as_uint(bs) > bounds[0]) atomicMax(&bounds[0], __float_as_uint(bs));
        if (__float_as_uint(bm) > bounds[1]) atomicMax(&bounds[1], __float_as_uint(bm));
    }
}
__global__ void k_fill_u32(int64_t n, uint32_t v, uint32_t* __restrict__ out) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) out[t] = v;
}

// the per-item arrays of a job (isim_front fills them): pair order, aux / inv_norm rank order
struct IsimItems {
    DevBuf<double> norm;                 // ||r_.i||
    DevBuf<double> sumsq;                // sum r^2 (Euclidean distance)
    DevBuf<double> centre, cnorm;        // Pearson: (sum |r|) / n and ||r - centre||
    DevBuf<float> colsum, colmax;        // full build: the bounds of the symmetric build's fixed-point scale
    DevBuf<double> aux;                  // a_i of the finishing measures
    DevBuf<double> inv_norm;             // 1 / ||r_.i|| (request: filled by the front; full build: by its packed walk)
};

// The symmetric build of a job that isim_route (fy_itemsim_plan.hpp) sent here.  false = gram_half_build declined (fixed-point
// scale, chunk count): the caller runs the row-at-a-time build.  cnt / other / sim as the other build leaves them.
static bool itemsim_symmetric(Context* ctx, const fy_itemsim_params* prm, const Prepared& P, const IsimItems& N, int32_t* cnt, int32_t* other, float* sim,
                              double* ms_cooc, fy_stats* st_out) {
    const Tuning& tune = ctx->tune;
    const int32_t Ic = P.nP, K = prm->max_similarities_per_item;
    const bool cosine = prm->similarity == FY_SIMILARITY_COSINE, counts = isim_measure(prm->similarity).counts;
    const double* aux = N.aux.get();
    const int64_t ldm = round_up(Ic, 256), slack = 1024;
    hipStream_t st = ctx->stream;
    DevBuf<double> invn(ctx, (size_t)Ic);
    DevBuf<float> invn32(ctx, (size_t)(ldm + slack));
    DevBuf<uint32_t> d_bounds(ctx, 2);
    d_bounds.zero();
    if (cosine)
        k_isim_gram_prep<<<grid_for(ldm + slack, 256, 256), 256, 0, st>>>(Ic, ldm + slack, P.rank_pair.get(), N.colsum.get(), N.colmax.get(), N.norm.get(), invn.get(), invn32.get(), d_bounds.get());
    else
        k_isim_gram_prep_aux<<<grid_for(ldm + slack, 256, 256), 256, 0, st>>>(Ic, ldm + slack, P.rank_pair.get(), N.colsum.get(), N.colmax.get(), aux, counts ? 1 : 0, invn32.get(), d_bounds.get());
    FY_KERNEL_CHECK();
    uint32_t hb[2];
    d2h(ctx, hb, d_bounds.get(), 2);
    sync(ctx);
    float fsum, fmax;
    memcpy(&fsum, &hb[0], 4);
    memcpy(&fmax, &hb[1], 4);
    const float bounds3[3] = {fsum, fmax, fmax};
    DevBuf<float> G(ctx, (size_t)Ic * ldm + slack);
    EventTimer t_all(ctx);
    const size_t sp = t_all.begin();
    double ms_tables = 0.0;
    DevBuf<float> ones(ctx, counts ? (size_t)P.nnz : 1);
    if (counts) {
        k_fill_u32<<<grid_for(P.nnz), 256, 0, st>>>(P.nnz, 0x3F800000u /* 1.0f */, reinterpret_cast<uint32_t*>(ones.get()));
        FY_KERNEL_CHECK();
    }
    if (!gram_half_build(ctx, P, counts ? ones.get() : P.csc_r.get(), bounds3, G.get(), ldm, &ms_tables, nullptr, counts ? ones.get() : nullptr)) return false;
    const int capg = tune.isim_capg;
    DevBuf<uint32_t> tau_g(ctx, (size_t)Ic);
    DevBuf<int32_t> gcnt(ctx, (size_t)Ic), overflow(ctx, (size_t)Ic);
    DevBuf<uint64_t> glist(ctx, (size_t)Ic * capg);
    gcnt.zero();
    overflow.zero();
    uint32_t tau0 = 1u;      // no threshold: similarity > 0 (NO_THRESHOLD = Double.MIN_VALUE)
    if (prm->has_threshold) {
        float tf = (float)prm->threshold;
        if ((double)tf < prm->threshold) tf = nextafterf(tf, INFINITY);      // float s >= double threshold  <=>  s >= the next float at or above it
        memcpy(&tau0, &tf, 4);
    }
    k_fill_u32<<<grid_for(Ic), 256, 0, st>>>(Ic, tau0, tau_g.get());
    FY_KERNEL_CHECK();
    DevBuf<uint32_t> hist_g(ctx, (size_t)round_up(Ic, 64) * 64);
    hist_g.zero();
    SweepArgs SA{G.get(), ldm, Ic, K, invn32.get(), cosine ? invn.get() : aux, (double)P.nU, P.rank_item_raw.get(), tau_g.get(), gcnt.get(), glist.get(), capg, overflow.get(),
                 hist_g.get(), (int32_t)ceil_div(Ic, 64), tune.isim_piece, tau0, prm->exclude_self, cnt, other, sim};
    const int npieces = (int)ceil_div(Ic, SA.piece);
    DevBuf<int32_t> redo_list(ctx, (size_t)Ic), n_redo(ctx, 1);
    n_redo.zero();
    isim_dispatch(prm->similarity, [&](auto M) {
        k_isim_sweep<decltype(M)::value><<<SA.nbands * npieces, 256, (size_t)(SA.piece + 256 + 64) * sizeof(float), st>>>(SA);
        FY_KERNEL_CHECK();
        k_isim_finish<decltype(M)::value><<<(int)ceil_div(SA.Ic, 4), 256, 0, st>>>(SA, redo_list.get(), n_redo.get());
        FY_KERNEL_CHECK();
        k_isim_redo<decltype(M)::value><<<ctx->num_cus * 2, 256, 0, st>>>(SA, redo_list.get(), n_redo.get());
        FY_KERNEL_CHECK();
    });
    t_all.end(sp);
    DevBuf<unsigned long long> d_cands(ctx, 1);
    d_cands.zero();
    k_sum_i32<<<grid_for(Ic), 256, 0, st>>>(Ic, gcnt.get(), d_cands.get());
    FY_KERNEL_CHECK();
    unsigned long long h_cands = 0;
    int32_t h_redo = 0;
    d2h(ctx, &h_cands, d_cands.get(), 1);
    d2h(ctx, &h_redo, n_redo.get(), 1);
    sync(ctx);
    *ms_cooc = t_all.total_ms() - ms_tables;
    st_out->ms_tables = ms_tables;
    st_out->isim_candidates = (int64_t)h_cands;
    st_out->isim_redone_rows = h_redo;
    return true;
}

// packed CSR (fy_cooc.hpp): column index relative to its chunk | the raw rating (or 1 for the co-occurrence count) as fp16
__global__ void k_isim_pack_csr(int64_t nnz, int32_t CH, const int32_t* __restrict__ csr_idx, const float* __restrict__ csr_r, int measure,
                                uint32_t* __restrict__ pk) {
    const bool rating = isim_measure(measure).weight == ISIM_W_RATING;
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < nnz; f += (int64_t)gridDim.x * blockDim.x)
        pk[f] = (uint32_t)(csr_idx[f] % CH) | ((uint32_t)__half_as_ushort(__float2half(rating ? csr_r[f] : 1.0f)) << 16);
}
__global__ void k_isim_raw_weights(int64_t nnz, const float* __restrict__ csc_r, int measure, float* __restrict__ csc_w) {
    const bool rating = isim_measure(measure).weight == ISIM_W_RATING;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * blockDim.x)
        csc_w[q] = rating ? csc_r[q] : 1.0f;
}
__global__ void k_isim_inv_norms(int32_t Ic, const int32_t* __restrict__ rank_pair, const double* __restrict__ norm, double* __restrict__ inv) {
    for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < Ic; r += gridDim.x * blockDim.x) inv[r] = 1.0 / norm[rank_pair[r]];
}

// a_i of the finishing measures in rank order: sum r^2 (Euclidean distance) or the number of raters (the count measures)
__global__ void k_isim_rank_norms(int32_t Ic, const int32_t* __restrict__ rank_pair, const int32_t* __restrict__ pair_start,
                                  const double* __restrict__ sumsq, double* __restrict__ aux) {
    for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < Ic; r += gridDim.x * blockDim.x) {
        const int32_t pr = rank_pair[r];
        aux[r] = sumsq ? sumsq[pr] : (double)(pair_start[pr + 1] - pair_start[pr]);
    }
}
__global__ void k_isim_count_heavy(int32_t rows_mine, int32_t rank, int32_t world, const int32_t* __restrict__ rank_pair,
                                   const int32_t* __restrict__ pair_start, int32_t heavy, int32_t* __restrict__ n_heavy) {
    for (int32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < rows_mine; m += gridDim.x * blockDim.x) {
        const int32_t pr = rank_pair[rank + m * world];
        if (pair_start[pr + 1] - pair_start[pr] > heavy) atomicAdd(n_heavy, 1);
    }
}

// ---- input preparation: minPrefsPerUser / maxPrefsPerUser (BaselinePreparePreferenceMatrixJob.java:104, 126-129; filmyou.h)
__global__ void k_pref_keys(int64_t n, const int32_t* __restrict__ user, const int32_t* __restrict__ item, uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        key[t] = ((uint64_t)(uint32_t)user[t] << 32) | (uint32_t)item[t];
        val[t] = (uint32_t)t;
    }
}
__global__ void k_pref_heads(int64_t n, const uint64_t* __restrict__ key, uint32_t* __restrict__ head) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x)
        head[p] = (p == 0 || (key[p] >> 32) != (key[p - 1] >> 32)) ? 1u : 0u;
}
__global__ void k_pref_head_pos(int64_t n, const uint32_t* __restrict__ head, const uint32_t* __restrict__ useq, uint32_t* __restrict__ head_pos) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p <= n; p += (int64_t)gridDim.x * blockDim.x) {
        if (p == n) head_pos[useq[n - 1]] = (uint32_t)n;          // sentinel behind the last user
        else if (head[p]) head_pos[useq[p] - 1] = (uint32_t)p;
    }
}
__global__ void k_pref_keep(int64_t n, const uint32_t* __restrict__ useq, const uint32_t* __restrict__ head_pos, int32_t min_prefs, int32_t max_prefs,
                            uint32_t* __restrict__ keep) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t u = useq[p] - 1;
        const int64_t first = head_pos[u], deg = (int64_t)head_pos[u + 1] - first, k = p - first;
        bool ok = deg >= min_prefs;
        if (ok && max_prefs > 0 && deg > max_prefs) ok = ((k + 1) * max_prefs) / deg > (k * max_prefs) / deg;
        keep[p] = ok ? 1u : 0u;
    }
}
__global__ void k_pref_emit(int64_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ off, const uint32_t* __restrict__ src,
                            const int32_t* __restrict__ user, const int32_t* __restrict__ item, const float* __restrict__ score,
                            int32_t* __restrict__ ou, int32_t* __restrict__ oi, float* __restrict__ os) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        if (!keep[p]) continue;
        const uint32_t t = src[p], o = off[p] - 1;
        ou[o] = user[t];
        oi[o] = item[t];
        os[o] = score[t];
    }
}
// a filtered copy of the ratings, or nullptr when neither option changes anything
static std::unique_ptr<fy_ratings> filter_user_prefs(Context* ctx, const fy_ratings* R, int32_t min_prefs, int32_t max_prefs) {
    if ((min_prefs <= 1 && max_prefs <= 0) || R->nnz == 0) return nullptr;
    if (R->nnz >= ((int64_t)1 << 32)) FY_FAIL(FY_ERR_UNSUPPORTED, "minPrefsPerUser / maxPrefsPerUser with more than 2^32 ratings");
    hipStream_t st = ctx->stream;
    const int64_t n = R->nnz;
    DevBuf<uint64_t> ka(ctx, n), kb(ctx, n);
    DevBuf<uint32_t> va(ctx, n), vb(ctx, n), head(ctx, n), useq(ctx, n), keep(ctx, n), off(ctx, n), head_pos(ctx, (size_t)n + 1);
    k_pref_keys<<<grid_for(n), 256, 0, st>>>(n, R->user.get(), R->item.get(), ka.get(), va.get());
    FY_KERNEL_CHECK();
    sort_pairs_u64_u32(ctx, ka.get(), kb.get(), va.get(), vb.get(), (size_t)n);
    k_pref_heads<<<grid_for(n), 256, 0, st>>>(n, kb.get(), head.get());
    FY_KERNEL_CHECK();
    inclusive_scan_u32(ctx, head.get(), useq.get(), (size_t)n);
    k_pref_head_pos<<<grid_for(n + 1), 256, 0, st>>>(n, head.get(), useq.get(), head_pos.get());
    FY_KERNEL_CHECK();
    k_pref_keep<<<grid_for(n), 256, 0, st>>>(n, useq.get(), head_pos.get(), min_prefs, max_prefs, keep.get());
    FY_KERNEL_CHECK();
    inclusive_scan_u32(ctx, keep.get(), off.get(), (size_t)n);
    const uint32_t kept = fetch(ctx, off.get() + (n - 1));
    std::unique_ptr<fy_ratings> F(new fy_ratings);
    F->ctx = ctx;
    F->nnz = kept;
    F->max_user = R->max_user;
    F->max_item = R->max_item;
    F->scores_fp16_exact = R->scores_fp16_exact;
    F->user.alloc(ctx, kept);
    F->item.alloc(ctx, kept);
    F->score.alloc(ctx, kept);
    k_pref_emit<<<grid_for(n), 256, 0, st>>>(n, keep.get(), off.get(), vb.get(), R->user.get(), R->item.get(), R->score.get(), F->user.get(),
                                             F->item.get(), F->score.get());
    FY_KERNEL_CHECK();
    sync(ctx);     // the scratch arrays of this function go back to the allocator
    return F;
}

// The front of both entry points: the checks in the order the full build has always made them (the input preparation's options
// before the preparation runs, the rest behind it), the filtered ratings, the structure, and the per-item arrays of the measure.
// false = no rating is left (P says so; nothing else is filled).  for_request: the prepared job -- no column bounds, 1 / norm for
// every epilogue.  t_total / t_prep: the full build's clocks (the whole job from here on; build_structure alone).
static bool isim_front(Context* ctx, const fy_itemsim_params* prm, const fy_ratings* R_in, bool for_request, Prepared& P, IsimItems& N,
                       EventTimer* t_total = nullptr, EventTimer* t_prep = nullptr) {
    if (prm->min_prefs_per_user < 0 || prm->max_prefs_per_user < 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "minPrefsPerUser / maxPrefsPerUser must be >= 0");
    const std::unique_ptr<fy_ratings> filtered = filter_user_prefs(ctx, R_in, prm->min_prefs_per_user, prm->max_prefs_per_user);
    if (prm->similarity < FY_SIMILARITY_COSINE || prm->similarity > FY_SIMILARITY_PEARSON_CORRELATION)
        FY_FAIL(FY_ERR_INVALID_ARGUMENT, "similarity must be one of the FY_SIMILARITY_* constants (0 .. %d)", (int)FY_SIMILARITY_PEARSON_CORRELATION);
    if (prm->similarity == FY_SIMILARITY_PEARSON_CORRELATION && prm->has_threshold && !(prm->threshold > 0.0))
        FY_FAIL(FY_ERR_UNSUPPORTED, "SIMILARITY_PEARSON_CORRELATION with a threshold <= 0: a co-rated pair whose centred products cancel to 0 "
                                    "cannot be told from a pair nobody co-rated");
    if (prm->max_similarities_per_item <= 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "maxSimilaritiesPerRow must be > 0");
    if (prm->max_similarities_per_item > ISIM_MAX_K)
        FY_FAIL(FY_ERR_UNSUPPORTED, "maxSimilaritiesPerRow %d exceeds the kernel limit %d", prm->max_similarities_per_item, ISIM_MAX_K);
    if (prm->world <= 0 || prm->rank < 0 || prm->rank >= prm->world) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "rank %d of world %d", prm->rank, prm->world);
    if (t_total) t_total->begin();
    const size_t sp = t_prep ? t_prep->begin() : 0;
    build_structure(ctx, filtered ? filtered.get() : R_in, 1, 0, nullptr, nullptr, nullptr, true, P);
    if (t_prep) t_prep->end(sp);
    if (P.nnz == 0) return false;
    if (prm->similarity == FY_SIMILARITY_EUCLIDEAN_DISTANCE && !P.ratings_positive)
        FY_FAIL(FY_ERR_UNSUPPORTED, "SIMILARITY_EUCLIDEAN_DISTANCE on data with a non-positive preference: a co-rated pair whose products sum to 0 "
                                    "cannot be told from a pair nobody co-rated");
    const IsimMeasure m = isim_measure(prm->similarity);
    const bool pearson = m.weight == ISIM_W_PEARSON, sumsq = m.a == ISIM_A_SUMSQ;
    const int32_t Ic = P.nP;   // single "cluster": every item is a pair
    hipStream_t st = ctx->stream;
    N.norm.alloc(ctx, Ic);
    N.inv_norm.alloc(ctx, Ic);
    if (!for_request) { N.colsum.alloc(ctx, Ic); N.colmax.alloc(ctx, Ic); }
    N.sumsq.alloc(ctx, sumsq ? Ic : 1);
    N.centre.alloc(ctx, pearson ? Ic : 1);
    N.cnorm.alloc(ctx, pearson ? Ic : 1);
    N.aux.alloc(ctx, m.finishes ? Ic : 1);
    // the norms, by one kernel in a fixed summation order: the full build and a request see the same bits
    const int norm_grid = std::min<int>(Ic, ctx->num_cus * 32);
    if (pearson)
        k_item_norms<true><<<norm_grid, 256, 0, st>>>(Ic, P.pair_start.get(), P.csc_r.get(), N.norm.get(), N.colsum.get(), N.colmax.get(), nullptr, N.centre.get(), N.cnorm.get());
    else
        k_item_norms<false><<<norm_grid, 256, 0, st>>>(Ic, P.pair_start.get(), P.csc_r.get(), N.norm.get(), N.colsum.get(), N.colmax.get(), sumsq ? N.sumsq.get() : nullptr,
                                                       nullptr, nullptr);
    FY_KERNEL_CHECK();
    if (m.finishes) {
        k_isim_rank_norms<<<grid_for(Ic), 256, 0, st>>>(Ic, P.rank_pair.get(), P.pair_start.get(), sumsq ? N.sumsq.get() : nullptr, N.aux.get());
        FY_KERNEL_CHECK();
    }
    if (for_request && m.inv_norm) {
        k_isim_inv_norms<<<grid_for(Ic), 256, 0, st>>>(Ic, P.rank_pair.get(), N.norm.get(), N.inv_norm.get());
        FY_KERNEL_CHECK();
    }
    return true;
}

// column chunks of the row-at-a-time kernel and every user's row offsets at their boundaries
struct IsimChunks {
    int32_t CH, nch, cap;
    DevBuf<int32_t> chunk_off;
};

// The row-at-a-time build of this rank's rows (rank, rank + world, ...): the weights of the walk the route names, the segment table,
// k_cooc_itemsim over (row, chunk) items, k_isim_merge.  Returns whether the row kernel ran (a rank without rows has nothing to build).
static bool itemsim_row_at_a_time(Context* ctx, const fy_itemsim_params* prm, const Prepared& P, IsimItems& N, bool use_pk, const IsimChunks& C, int32_t rows_mine,
                                  int32_t* cnt, int32_t* other, float* sim, EventTimer& t_cooc) {
    const Tuning& tune = ctx->tune;
    hipStream_t st = ctx->stream;
    const int measure = prm->similarity;
    const IsimMeasure m = isim_measure(measure);
    const int32_t Ic = P.nP, K = prm->max_similarities_per_item, CH = C.CH, nch = C.nch;
    DevBuf<float> csc_w(ctx, (size_t)P.nnz), csr_w(ctx, use_pk ? 1 : (size_t)P.nnz);
    DevBuf<uint32_t> csr_pk(ctx, use_pk ? (size_t)P.nnz : 1);
    if (use_pk) {
        k_isim_raw_weights<<<grid_for(P.nnz), 256, 0, st>>>(P.nnz, P.csc_r.get(), measure, csc_w.get());
        FY_KERNEL_CHECK();
        if (m.inv_norm) {
            k_isim_inv_norms<<<grid_for(Ic), 256, 0, st>>>(Ic, P.rank_pair.get(), N.norm.get(), N.inv_norm.get());
            FY_KERNEL_CHECK();
        }
    } else {
        const double* wnorm = m.weight == ISIM_W_PEARSON ? N.cnorm.get() : N.norm.get();      // the norm the pre-divided weights use
        k_csc_weights<<<grid_for(P.nnz), 256, 0, st>>>(P.nnz, P.csc_pair.get(), P.csc_r.get(), wnorm, N.centre.get(), measure, csc_w.get());
        FY_KERNEL_CHECK();
        k_csr_weights<<<grid_for(P.nnz), 256, 0, st>>>(P.nnz, P.csr_idx.get(), P.csr_r.get(), P.rank_pair.get(), wnorm, N.centre.get(), measure, csr_w.get());
        FY_KERNEL_CHECK();
    }
    if (rows_mine <= 0) return false;
    SegStore segs;
    const SegDesc sd = seg_desc(0, 0, (int32_t)P.nnz, nch);
    build_segment_table(ctx, SegArrays{P.csc_slot.get(), csc_w.get(), C.chunk_off.get(), nullptr, nullptr}, sd, segs);
    if (use_pk) {
        k_isim_pack_csr<<<grid_for(P.nnz), 256, 0, st>>>(P.nnz, CH, P.csr_idx.get(), P.csr_r.get(), measure, csr_pk.get());
        FY_KERNEL_CHECK();
    }
    CoocArgs CA = cooc_args(P, segs.view(sd), CoocGeometry{0, 0, Ic, CH, nch, 0, (int32_t)P.nnz}, csr_w.get(), use_pk ? csr_pk.get() : nullptr);
    CA.row0 = prm->rank; CA.nrows = rows_mine; CA.row_stride = prm->world;      // this rank's rows: rank, rank + world, ...
    DevBuf<int2> item_seg(ctx, (size_t)rows_mine * nch);
    DevBuf<int32_t> part_cnt(ctx, (size_t)rows_mine * nch);
    part_cnt.zero();
    // rows are in popularity order: the rows with more than ISIM_HEAVY raters are a prefix
    DevBuf<int32_t> d_heavy(ctx, 1);
    d_heavy.zero();
    k_isim_count_heavy<<<grid_for(rows_mine), 256, 0, st>>>(rows_mine, prm->rank, prm->world, P.rank_pair.get(), P.pair_start.get(), tune.isim_heavy, d_heavy.get());
    FY_KERNEL_CHECK();
    const int32_t heavy_rows = nch > 1 ? fetch(ctx, d_heavy.get()) : 0;
    const int64_t n_items = (int64_t)heavy_rows * nch + (rows_mine - heavy_rows);
    DevBuf<uint64_t> part(ctx, (size_t)rows_mine * nch * K);
    k_item_segments<<<grid_for((int64_t)rows_mine * nch), 256, 0, st>>>(CA, item_seg.get());
    FY_KERNEL_CHECK();
    CA.item_seg = item_seg.get();
    ISimEpilogue IE{P.rank_item_raw.get(), K, prm->exclude_self, prm->has_threshold, (float)prm->threshold, prm->rank,
                    prm->world, cnt, other, sim, (use_pk && m.inv_norm) ? N.inv_norm.get() : nullptr,
                    m.finishes ? N.aux.get() : nullptr, (double)P.nU, part_cnt.get(), part.get(), heavy_rows, (int32_t)n_items, C.cap};
    const size_t lds = (size_t)CH * 8 + (size_t)C.cap * 8;
    const int block = lds > 48 * 1024 ? 1024 : 256;
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2048 / block, (160 * 1024) / (lds + 1024)));
    const int grid = (int)std::min<int64_t>(n_items, (int64_t)ctx->num_cus * per_cu);
    DevBuf<int32_t> next_row(ctx, 1);
    next_row.zero();
    const size_t sp = t_cooc.begin();
    isim_dispatch(measure, [&](auto M) {
        const auto kernel = use_pk ? k_cooc_itemsim<true, decltype(M)::value> : k_cooc_itemsim<false, decltype(M)::value>;
        FY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        kernel<<<grid, block, lds, st>>>(CA, IE, next_row.get());
        FY_KERNEL_CHECK();
    });
    k_isim_merge<<<std::min(rows_mine, ctx->num_cus * 8), 256, 0, st>>>(rows_mine, nch, K, part_cnt.get(), part.get(), cnt, other, sim);
    FY_KERNEL_CHECK();
    t_cooc.end(sp);
    sync(ctx);   // part / item_seg go back to the allocator at the end of this scope
    return true;
}

// n rows for a result of kind 1: (item, other item, similarity, 0)
void isim_result_rows(fy_result* R, int64_t n) {
    R->n = n;
    for (DevBuf<int32_t>* b : {&R->d_key0, &R->d_key1, &R->d_aux}) b->alloc(R->ctx, (size_t)n);
    R->d_value.alloc(R->ctx, (size_t)n);
}
// the empty result of kind 1 (item similarities) over the job's structure: what both entry points and the request pass start from
std::unique_ptr<fy_result> isim_empty_result(Context* ctx, const Prepared& P) {
    std::unique_ptr<fy_result> R(new fy_result);
    R->ctx = ctx;
    R->kind = 1;
    R->st.nnz = P.nnz;
    R->st.n_users = P.nU;
    R->st.n_items = P.nI;
    isim_result_rows(R.get(), 0);
    R->d_user_id.alloc(ctx, 0);
    R->d_item_id.alloc(ctx, 0);
    return R;
}

// front, route, one of the two builds, compact, statistics
fy_result* itemsim_build(Context* ctx, const fy_itemsim_params* prm, const fy_ratings* R_in) {
    EventTimer t_prep(ctx), t_cooc(ctx), t_total(ctx);
    Prepared P;
    IsimItems N;
    const bool any = isim_front(ctx, prm, R_in, false, P, N, &t_total, &t_prep);
    std::unique_ptr<fy_result> Rs = isim_empty_result(ctx, P);
    hipStream_t st = ctx->stream;
    if (!any) { t_total.end(0); sync(ctx); return Rs.release(); }
    const Tuning& tune = ctx->tune;
    const int32_t Ic = P.nP, K = prm->max_similarities_per_item;
    const IsimRoute route = isim_route({prm->similarity, K, prm->world, prm->has_threshold != 0, prm->threshold, Ic, P.ratings_fp16_exact, P.ratings_positive,
                                        (uint64_t)ctx->total_mem, tune.isim_gram, tune.isim_gram_min_items, tune.cooc_pk});
    const int32_t rows_mine = (Ic - prm->rank + prm->world - 1) / prm->world;
    DevBuf<int32_t> cnt(ctx, (size_t)rows_mine + 1), off(ctx, (size_t)rows_mine + 1), other(ctx, (size_t)rows_mine * K);
    DevBuf<float> sim(ctx, (size_t)rows_mine * K);
    cnt.zero();
    double ms_sym = 0.0;
    const bool symmetric = route.symmetric && itemsim_symmetric(ctx, prm, P, N, cnt.get(), other.get(), sim.get(), &ms_sym, &Rs->st);
    // LDS = fp64 accumulators + candidate buffer <= 160 KiB.  (A 512-entry buffer would allow three column chunks instead of
    // four at ML-25M shape, but the extra cuts cost more than the shorter walk gains: 28.5 against 27.2 ms.)
    IsimChunks C;
    C.cap = ISIM_CAP;
    int max_ch = ((160 * 1024 - C.cap * 8 - 2048) / 8) / 256 * 256;
    if (tune.cooc_max_ch_forced && tune.cooc_max_ch <= max_ch) max_ch = tune.cooc_max_ch;   // test hook: force column chunks
    pick_chunks(Ic, max_ch, C.CH, C.nch);
    C.chunk_off.alloc(ctx, (size_t)P.nU * (C.nch + 1));
    const CsrDescs cd = upload_csr_descs(ctx, {csr_desc(0, P.nU, C.CH, C.nch)});
    build_chunk_offsets(ctx, cd, P.rowptr.get(), P.csr_idx.get(), C.chunk_off.get());
    if (symmetric || itemsim_row_at_a_time(ctx, prm, P, N, route.packed, C, rows_mine, cnt.get(), other.get(), sim.get(), t_cooc)) Rs->st.cooc_launches = 1;
    exclusive_scan_i32(ctx, cnt.get(), off.get(), (size_t)rows_mine + 1);
    const int64_t n = fetch(ctx, off.get() + rows_mine);
    isim_result_rows(Rs.get(), n);
    if (rows_mine > 0 && n > 0) {
        k_isim_compact<<<grid_for((int64_t)rows_mine * 64, 256), 256, 0, st>>>(rows_mine, K, nullptr, prm->rank, prm->world, cnt.get(), off.get(), other.get(), sim.get(),
                                                                               P.rank_item_raw.get(), Rs->d_key0.get(), Rs->d_key1.get(), Rs->d_value.get(), Rs->d_aux.get());
        FY_KERNEL_CHECK();
    }
    t_total.end(0);
    sync(ctx);
    Rs->st.recs = n;
    Rs->st.pair_contribs = P.sum_deg2;
    // sum_u n_u (n_u - 1) / 2 = (sum n_u^2 - nnz) / 2: the unit Mahout's co-occurrence mapper enumerates
    Rs->st.unordered_pairs = (P.sum_deg2 - P.nnz) / 2;
    Rs->st.ms_prepare = t_prep.total_ms();
    Rs->st.ms_cooc = symmetric ? ms_sym : t_cooc.total_ms();
    Rs->st.ms_total = t_total.total_ms();
    return Rs.release();
}

// ================================================================ the prepared job (fy_itemsim_prepare; requests: fy_itemsim_request.hip)
// per item in rank order: the sum of the raters' degrees (what a request for the item walks), one wave per item
__global__ void k_isim_req_walk(int32_t Ic, const int32_t* __restrict__ rank_pair, const int32_t* __restrict__ pair_start,
                                const int32_t* __restrict__ csc_slot, const int32_t* __restrict__ rowptr, long long* __restrict__ walk) {
    const int wpb = blockDim.x >> 6, lane = threadIdx.x & 63;
    for (int32_t r = blockIdx.x * wpb + (threadIdx.x >> 6); r < Ic; r += gridDim.x * wpb) {
        const int32_t pr = rank_pair[r];
        long long s = 0;
        for (int32_t q = pair_start[pr] + lane; q < pair_start[pr + 1]; q += 64) {
            const int32_t v = csc_slot[q];
            s += rowptr[v + 1] - rowptr[v];
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0) walk[r] = s;
    }
}
// Pearson in fp64: the centred, normalised preference of every CSR entry (0 on a constant item, whose pairs drop out through unit[])
__global__ void k_isim_req_pearson_weights(int64_t nnz, const int32_t* __restrict__ csr_idx, const float* __restrict__ csr_r,
                                           const int32_t* __restrict__ rank_pair, const double* __restrict__ centre, const double* __restrict__ cnorm,
                                           double* __restrict__ csr_w) {
    for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < nnz; f += (int64_t)gridDim.x * blockDim.x) {
        const int32_t p = rank_pair[csr_idx[f]];
        const double cn = cnorm[p];
        csr_w[f] = cn != 0.0 ? ((double)csr_r[f] - centre[p]) * (1.0 / cn) : 0.0;
    }
}
// ... and per item in rank order the factor of its similarities: 1, NaN for a constant item (0 / 0 in the statement)
__global__ void k_isim_req_pearson_unit(int32_t Ic, const int32_t* __restrict__ rank_pair, const double* __restrict__ cnorm, double* __restrict__ unit) {
    for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < Ic; r += gridDim.x * blockDim.x)
        unit[r] = cnorm[rank_pair[r]] != 0.0 ? 1.0 : __longlong_as_double(0x7FF8000000000000ll);
}

fy_itemsim_job* itemsim_prepare(Context* ctx, const fy_itemsim_params* prm, const fy_ratings* R_in) {
    std::unique_ptr<fy_itemsim_job> J(new fy_itemsim_job);
    J->ctx = ctx;
    J->prm = *prm;
    Prepared& P = J->P;
    IsimItems N;
    if (!isim_front(ctx, prm, R_in, true, P, N)) { sync(ctx); return J.release(); }
    hipStream_t st = ctx->stream;
    const int32_t Ic = P.nP;
    const IsimMeasure m = isim_measure(prm->similarity);
    const bool pearson = m.weight == ISIM_W_PEARSON;
    // the job owns what its requests read; the norms themselves are only needed for the bounds below
    J->centre = std::move(N.centre);
    J->cnorm = std::move(N.cnorm);
    J->inv_norm = std::move(N.inv_norm);
    J->aux = std::move(N.aux);
    J->csr_w.alloc(ctx, pearson ? (size_t)P.nnz : 1);
    if (pearson) {
        k_isim_req_pearson_weights<<<grid_for(P.nnz), 256, 0, st>>>(P.nnz, P.csr_idx.get(), P.csr_r.get(), P.rank_pair.get(), J->centre.get(), J->cnorm.get(),
                                                                   J->csr_w.get());
        FY_KERNEL_CHECK();
        k_isim_req_pearson_unit<<<grid_for(Ic), 256, 0, st>>>(Ic, P.rank_pair.get(), J->cnorm.get(), J->inv_norm.get());
        FY_KERNEL_CHECK();
    }
    // the request kernel's column chunks and every user's row offsets at their boundaries
    // (FY_ISIM_REQ_CHUNK is the widest chunk; the chunks of a row are balanced: ML-25M shape, 59 047 columns = 8 chunks of 7424, whose
    // 58 KiB of accumulators + 16 KiB of candidates + 1 KiB of static LDS let two workgroups share a CU -- at the full 8192 only one fits)
    J->nch = (int32_t)ceil_div(Ic, std::min<int64_t>(ctx->tune.isim_req_chunk, round_up(Ic, 64)));
    J->CH = (int32_t)round_up(ceil_div(Ic, J->nch), 64);
    J->choff.alloc(ctx, (size_t)P.nU * (size_t)(J->nch + 1));
    const CsrDescs cd = upload_csr_descs(ctx, {csr_desc(0, P.nU, J->CH, J->nch)});
    build_chunk_offsets(ctx, cd, P.rowptr.get(), P.csr_idx.get(), J->choff.get());
    DevBuf<long long> d_walk(ctx, Ic);
    k_isim_req_walk<<<grid_for((int64_t)Ic * 64, 256), 256, 0, st>>>(Ic, P.rank_pair.get(), P.pair_start.get(), P.csc_slot.get(), P.rowptr.get(), d_walk.get());
    FY_KERNEL_CHECK();
    // host mirrors a request is planned from: raw ids ascending -> popularity rank, the walk per rank; and the bound of every row's
    // entries for the fixed-point scale: |d_ji| <= ||w_.j|| ||w_.i|| (Cauchy-Schwarz) <= ||w_.j|| max_i ||w_.i||, which is
    // n_j for the count measures (w = 1, d_ji <= n_j) and 1 for Pearson's normalised columns
    std::vector<int32_t> raw((size_t)Ic), rank_pair((size_t)Ic), pair_start((size_t)Ic + 1);
    std::vector<double> h_norm((size_t)Ic), h_bound((size_t)Ic);
    J->walk.resize((size_t)Ic);
    d2h(ctx, raw.data(), P.rank_item_raw.get(), (size_t)Ic);
    d2h(ctx, rank_pair.data(), P.rank_pair.get(), (size_t)Ic);
    d2h(ctx, pair_start.data(), P.pair_start.get(), (size_t)Ic + 1);
    d2h(ctx, h_norm.data(), N.norm.get(), (size_t)Ic);
    d2h(ctx, J->walk.data(), d_walk.get(), (size_t)Ic);
    sync(ctx);
    std::vector<std::pair<int32_t, int32_t>> by_raw((size_t)Ic);
    for (int32_t r = 0; r < Ic; r++) by_raw[(size_t)r] = {raw[(size_t)r], r};
    std::sort(by_raw.begin(), by_raw.end());
    J->raw_sorted.resize((size_t)Ic);
    J->rank_of_sorted.resize((size_t)Ic);
    for (int32_t k = 0; k < Ic; k++) { J->raw_sorted[(size_t)k] = by_raw[(size_t)k].first; J->rank_of_sorted[(size_t)k] = by_raw[(size_t)k].second; }
    double max_norm = 0.0;
    for (double x : h_norm) max_norm = std::max(max_norm, x);
    for (int32_t r = 0; r < Ic; r++) {
        const int32_t pr = rank_pair[(size_t)r];
        h_bound[(size_t)r] = pearson ? 1.0 : m.weight == ISIM_W_RATING ? h_norm[(size_t)pr] * max_norm : (double)(pair_start[(size_t)pr + 1] - pair_start[(size_t)pr]);
    }
    J->bound.alloc(ctx, Ic);
    h2d(ctx, J->bound.get(), h_bound.data(), (size_t)Ic);
    sync(ctx);      // the host sources of the upload and the scratch of this function go away
    return J.release();
}

}  // namespace fy
