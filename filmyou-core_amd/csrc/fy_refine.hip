// fy_refine.hip -- cluster refinement (the reference's --usersPerSubCluster / -k2 stage) in one batched pass.
//
// Replaces (M = es/udc/fi/dc/irlab):
//   M/rmrecommender/RMRecommenderDriver.java:217-266 (clusterRefinement), :298-345 (doMappings)
//   M/nmf/clustering/SubClusterMappingJob.java + UserMappingReducer / ItemMappingReducer      new ids per parent cluster
//   M/nmf/common/MappingsMapper.java / MappingsReducer.java                                    the id lookups of the sub-runs
//   one PPCDriver (or NMFDriver) run per parent cluster, random initial matrices
//   M/nmf/clustering/ClusterAssignmentJob(true) + FindSubClusterMapper.java:46-76
//
// All parent clusters advance together.  Rows (users / items of all clusters) are numbered cluster-major, inside a cluster by
// ascending raw id; the factor matrices are ragged: cluster c owns n_c x k_c doubles of H and m_c x k_c of W, one after the
// other.  The rating matrix is block diagonal in these row numbers, so one CSR / CSC serves every cluster and an entry's
// column is a global row number of the other side.  k_c is small (ceil(n_c / usersPerSubCluster): 4-16 typically), so a wave
// is shared by 64 / L rows (or row chunks), L = the power of two >= k_c: lane % L is the column.  Every sum has a fixed
// order, two runs give the same bits.
#include <algorithm>
#include <cfloat>
#include <vector>

#include "fy_common.hpp"
#include "fy_prep.hpp"
#include "fy_refine.hpp"

namespace fy {

namespace {

constexpr int RF_MAX_K = 256;      // the limit of fy_nmf.hip
constexpr int RF_CHUNK = 256;      // entries of a row one lane group walks; longer rows are cut, partials added in chunk order
constexpr int RF_GRAM_ROWS = 128;  // least rows per partial Gram block
constexpr int RF_GRAM_BLOCKS = 256;   // most partial Gram blocks per cluster

inline int rf_grid(int64_t n, int block = 256, int cap = 4096) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, block), cap));
}

// one side (users with H, or items with W) of one parent cluster
struct RfSeg {
    int32_t row0, nrows;       // global rows of the cluster
    int32_t k, L;              // columns; lanes per row (power of two, 64 when k > 64)
    int32_t chunk0, nchunks;   // row chunks of the cluster's CSR rows
    int32_t gram_rows, gram_nb;   // rows per partial Gram block, number of blocks
    int64_t moff;              // first element of the cluster's factor matrix in the ragged array
    int64_t poff;              // first element of the cluster's chunk partials (nchunks x k)
    int64_t goff;              // first element of the cluster's k x k matrix
    int64_t gpoff;             // first element of the cluster's partial Gram blocks (gram_nb x k x k)
};

// the cluster whose range [base[c], base[c + 1]) holds w (base ascending, base[0] = 0, w < base[K])
__device__ __forceinline__ int32_t rf_find(const int32_t* __restrict__ base, int32_t K, int32_t w) {
    int32_t lo = 0, hi = K;      // invariant: base[lo] <= w < base[hi]
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (base[mid] <= w) lo = mid; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------- mappings
__global__ void k_rf_last_entry(int64_t n_map, const int32_t* __restrict__ map_user, int32_t* __restrict__ last) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_map; t += (int64_t)gridDim.x * blockDim.x)
        atomicMax(&last[map_user[t]], (int32_t)t);
}

// cl_of_raw[u] = cluster of the user's LAST map entry, -1 when the map does not name u; member keys (cluster << 32 | u)
__global__ void k_rf_cluster_of_raw(int32_t n_tab, const int32_t* __restrict__ last, const int32_t* __restrict__ map_cluster, int32_t K,
                                    int32_t* __restrict__ cl_of_raw, uint64_t* __restrict__ keys, int32_t* __restrict__ n_members,
                                    int* __restrict__ err) {
    for (int32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < n_tab; u += gridDim.x * blockDim.x) {
        const int32_t e = last[u];
        int32_t c = -1;
        uint64_t key = ~0ull;
        if (e >= 0) {
            c = map_cluster[e];
            if (c < 0 || c >= K) { atomicOr(err, 1); c = -1; }
            else { key = ((uint64_t)(uint32_t)c << 32) | (uint32_t)u; atomicAdd(n_members, 1); }
        }
        cl_of_raw[u] = c;
        keys[u] = key;
    }
}

__global__ void k_rf_user_rows(int32_t n_rows, const uint64_t* __restrict__ keys, int32_t* __restrict__ user_raw, int32_t* __restrict__ user_cl,
                               int32_t* __restrict__ row_of_raw) {
    for (int32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n_rows; g += gridDim.x * blockDim.x) {
        const uint64_t key = keys[g];
        const int32_t u = (int32_t)(uint32_t)key;
        user_raw[g] = u;
        user_cl[g] = (int32_t)(key >> 32);
        row_of_raw[u] = g;
    }
}

// ptr[r] = first sorted key whose high word is >= r, r in [0, n_seg]
__global__ void k_rf_segptr(int32_t n_seg, int64_t n, const uint64_t* __restrict__ keys, int32_t* __restrict__ ptr) {
    for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r <= n_seg; r += gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)(keys[mid] >> 32) < (int64_t)r) lo = mid + 1; else hi = mid;
        }
        ptr[r] = (int32_t)lo;
    }
}

// items of cluster c: rated with score > 0 by a user whose getCluster is c; a user the map does not name has cluster 0
// (ItemByClusterHDFSMapper.java:38-43, AbstractByClusterMapper.java:77-79)
__global__ void k_rf_item_presence(int64_t n, const int32_t* __restrict__ user, const int32_t* __restrict__ item, const float* __restrict__ score,
                                   int32_t n_tab, const int32_t* __restrict__ cl_of_raw, int32_t K, int32_t I, int32_t* __restrict__ pres,
                                   int* __restrict__ err) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        if (!(score[t] > 0.0f)) continue;
        const int32_t u = user[t], i = item[t];
        if (u < 0 || i < 0 || i >= I) { atomicOr(err, 2); continue; }
        int32_t c = u < n_tab ? cl_of_raw[u] : -1;
        if (c < 0) c = 0;
        if (c < K) pres[(int64_t)c * I + i] = 1;
    }
}

__global__ void k_rf_item_rows(int32_t K, int32_t I, const int32_t* __restrict__ ipos, int32_t* __restrict__ item_raw, int32_t* __restrict__ item_cl,
                               int32_t* __restrict__ istart) {
    const int64_t total = (int64_t)K * I;
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
        const int32_t gi = ipos[x];
        if (ipos[x + 1] > gi) {
            item_raw[gi] = (int32_t)(x % I);
            item_cl[gi] = (int32_t)(x / I);
        }
        if (x % I == 0) istart[x / I] = gi;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) istart[K] = ipos[total];
}

// a rating is kept when its user has a new id in its cluster and its item one too (VectorByItemHDFSMapper.java:48-52,
// ItemScoreByUserHDFSMapper.java:46-49): score > 0 and the user is a member -- its items are then in the cluster's item set
__global__ void k_rf_keys(int64_t n, const int32_t* __restrict__ user, const int32_t* __restrict__ item, const float* __restrict__ score,
                          int32_t n_tab, const int32_t* __restrict__ cl_of_raw, const int32_t* __restrict__ row_of_raw, int32_t I,
                          const int32_t* __restrict__ ipos, uint64_t* __restrict__ by_user, uint64_t* __restrict__ by_item,
                          unsigned long long* __restrict__ kept) {
    unsigned long long local = 0;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        uint64_t ku = ~0ull, ki = ~0ull;
        if (score[t] > 0.0f) {
            const int32_t u = user[t], i = item[t];
            const int32_t c = (u >= 0 && u < n_tab) ? cl_of_raw[u] : -1;
            if (c >= 0 && i >= 0 && i < I) {
                const uint32_t g = (uint32_t)row_of_raw[u], gi = (uint32_t)ipos[(int64_t)c * I + i];
                ku = ((uint64_t)g << 32) | gi;
                ki = ((uint64_t)gi << 32) | g;
                local++;
            }
        }
        by_user[t] = ku;
        by_item[t] = ki;
    }
    for (int o = 32; o > 0; o >>= 1) local += __shfl_down(local, o, 64);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(kept, local);
}

// first row without an entry; rows of a parent cluster without users are passed over (its sub-run factorises nothing)
__global__ void k_rf_first_empty(int32_t n_rows, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ row_cl,
                                 const int32_t* __restrict__ ustart, int32_t* __restrict__ first_empty) {
    for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += gridDim.x * blockDim.x) {
        const int32_t c = row_cl[r];
        if (rowptr[r + 1] == rowptr[r] && ustart[c + 1] > ustart[c]) atomicMin(first_empty, r);
    }
}

// ---------------------------------------------------------------- chunk tables
__global__ void k_rf_chunk_counts(int32_t n_rows, const int32_t* __restrict__ rowptr, int32_t* __restrict__ cnt) {
    for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r <= n_rows; r += gridDim.x * blockDim.x)
        cnt[r] = r < n_rows ? (rowptr[r + 1] - rowptr[r] + RF_CHUNK - 1) / RF_CHUNK : 0;
}
__global__ void k_rf_chunk_rows(int32_t n_rows, const int32_t* __restrict__ chunkptr, int32_t* __restrict__ chunk_row) {
    for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += gridDim.x * blockDim.x)
        for (int32_t c = chunkptr[r]; c < chunkptr[r + 1]; c++) chunk_row[c] = r;
}

// ---------------------------------------------------------------- initial matrices
__host__ __device__ __forceinline__ uint64_t rf_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// include/filmyou.h, fy_cluster_refine: the value of element (row, col) of matrix `which` (0 = H, 1 = W) of parent cluster c
__host__ __device__ __forceinline__ double rf_initial(uint64_t seed, uint32_t c, uint32_t which, uint32_t row, uint32_t col) {
    const uint64_t a = rf_splitmix64(((uint64_t)row << 32) | col);
    const uint64_t b = rf_splitmix64((((uint64_t)c << 32) | which) ^ a);
    const uint64_t z = rf_splitmix64(seed ^ b);
    return (double)((z >> 11) + 1) * 0x1.0p-53;     // (0, 1]
}

__global__ void k_rf_init(int32_t n_waves, int32_t K, const int32_t* __restrict__ rwave, const RfSeg* __restrict__ seg, uint64_t seed,
                          uint32_t which, double* __restrict__ M) {
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int32_t w = blockIdx.x * wpb + (threadIdx.x >> 6); w < n_waves; w += gridDim.x * wpb) {
        const int32_t c = rf_find(rwave, K, w);
        const RfSeg S = seg[c];
        const int32_t rl = (w - rwave[c]) * (64 / S.L) + lane / S.L;
        if (rl >= S.nrows) continue;
        for (int32_t col = lane % S.L; col < S.k; col += 64)
            M[S.moff + (int64_t)rl * S.k + col] = rf_initial(seed, (uint32_t)c, which, (uint32_t)rl, (uint32_t)col);
    }
}

// ---------------------------------------------------------------- the iteration
// SpMM, first stage: part[chunk][:] = sum over the chunk's entries a * B[col][:], entries in order.  64 / L chunks per wave.
__global__ void __launch_bounds__(256)
k_rf_spmm(int32_t n_waves, int32_t K, const int32_t* __restrict__ swave, const RfSeg* __restrict__ seg, const RfSeg* __restrict__ segB,
          const int32_t* __restrict__ chunk_row, const int32_t* __restrict__ chunkptr, const int32_t* __restrict__ rowptr,
          const uint64_t* __restrict__ keys, const float* __restrict__ val, const double* __restrict__ B, double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int32_t w = blockIdx.x * wpb + (threadIdx.x >> 6); w < n_waves; w += gridDim.x * wpb) {
        const int32_t c = rf_find(swave, K, w);
        const RfSeg S = seg[c];
        const int32_t k = S.k;
        const int32_t chl = (w - swave[c]) * (64 / S.L) + lane / S.L, col = lane % S.L;
        if (chl >= S.nchunks) continue;
        const int32_t ch = S.chunk0 + chl, r = chunk_row[ch];
        const int32_t f0 = rowptr[r] + (ch - chunkptr[r]) * RF_CHUNK, f1 = min(rowptr[r + 1], f0 + RF_CHUNK);
        const double* __restrict__ Bc = B + segB[c].moff;
        const int32_t brow0 = segB[c].row0;
        double* __restrict__ out = part + S.poff + (int64_t)chl * k;
        if (k <= 64) {
            double acc = 0.0;
            if (col < k) {
                int32_t f = f0;
                for (; f + 4 <= f1; f += 4) {      // four gathers in flight, added in entry order
                    const double v0 = Bc[(int64_t)((int32_t)(uint32_t)keys[f] - brow0) * k + col];
                    const double v1 = Bc[(int64_t)((int32_t)(uint32_t)keys[f + 1] - brow0) * k + col];
                    const double v2 = Bc[(int64_t)((int32_t)(uint32_t)keys[f + 2] - brow0) * k + col];
                    const double v3 = Bc[(int64_t)((int32_t)(uint32_t)keys[f + 3] - brow0) * k + col];
                    acc += (double)val[f] * v0;
                    acc += (double)val[f + 1] * v1;
                    acc += (double)val[f + 2] * v2;
                    acc += (double)val[f + 3] * v3;
                }
                for (; f < f1; f++) acc += (double)val[f] * Bc[(int64_t)((int32_t)(uint32_t)keys[f] - brow0) * k + col];
                out[col] = acc;
            }
        } else {
            double acc[RF_MAX_K / 64];
#pragma unroll
            for (int x = 0; x < RF_MAX_K / 64; x++) acc[x] = 0.0;
            for (int32_t f = f0; f < f1; f++) {
                const double a = (double)val[f];
                const double* __restrict__ b = Bc + (int64_t)((int32_t)(uint32_t)keys[f] - brow0) * k;
#pragma unroll
                for (int x = 0; x < RF_MAX_K / 64; x++) {
                    const int cc = col + 64 * x;
                    if (cc < k) acc[x] += a * b[cc];
                }
            }
#pragma unroll
            for (int x = 0; x < RF_MAX_K / 64; x++) {
                const int cc = col + 64 * x;
                if (cc < k) out[cc] = acc[x];
            }
        }
    }
}

// C_c = M_c^T M_c, first stage: a workgroup sums a contiguous row range of one cluster.  Small k: the workgroup's threads are
// 256 / pow2(k^2) row slices x k^2 elements, the slices are added in slice order through LDS.
__global__ void __launch_bounds__(256)
k_rf_gram_partial(int32_t K, const int32_t* __restrict__ gblock, const RfSeg* __restrict__ seg, const double* __restrict__ M,
                  double* __restrict__ part) {
    __shared__ double sh[256];
    const int32_t b = blockIdx.x;
    const int32_t c = rf_find(gblock, K, b);
    const RfSeg S = seg[c];
    const int32_t bl = b - gblock[c], k = S.k, E = k * k;
    const int32_t r0 = bl * S.gram_rows, r1 = min(S.nrows, r0 + S.gram_rows);
    const double* __restrict__ Mc = M + S.moff;
    double* __restrict__ out = part + S.gpoff + (int64_t)bl * E;
    if (E <= 128) {
        int Ep = 1;
        while (Ep < E) Ep <<= 1;
        const int slices = 256 / Ep, sl = threadIdx.x / Ep, e = threadIdx.x % Ep;
        double s = 0.0;
        if (e < E) {
            const int a = e / k, bb = e % k;
            for (int32_t r = r0 + sl; r < r1; r += slices) s += Mc[(int64_t)r * k + a] * Mc[(int64_t)r * k + bb];
        }
        sh[threadIdx.x] = s;
        __syncthreads();
        if ((int)threadIdx.x < E) {
            double t = 0.0;
            for (int q = 0; q < slices; q++) t += sh[q * Ep + threadIdx.x];
            out[threadIdx.x] = t;
        }
    } else {
        for (int e = threadIdx.x; e < E; e += blockDim.x) {
            const int a = e / k, bb = e % k;
            double s = 0.0;
            for (int32_t r = r0; r < r1; r++) s += Mc[(int64_t)r * k + a] * Mc[(int64_t)r * k + bb];
            out[e] = s;
        }
    }
}
// second stage: the cluster's blocks in block order.  grid (K, y)
__global__ void k_rf_gram_sum(const RfSeg* __restrict__ seg, const double* __restrict__ part, double* __restrict__ C) {
    const RfSeg S = seg[blockIdx.x];
    const int32_t E = S.k * S.k;
    for (int32_t e = blockIdx.y * blockDim.x + threadIdx.x; e < E; e += gridDim.y * blockDim.x) {
        double s = 0.0;
        for (int32_t p = 0; p < S.gram_nb; p++) s += part[S.gpoff + (int64_t)p * E + e];
        C[S.goff + e] = s;
    }
}

__device__ __forceinline__ double rf_clampinf(double v) { return isinf(v) ? (v > 0 ? DBL_MAX : -DBL_MAX) : v; }

// out[r][c] = m_c * x_c / (y_c + eps), y = C m, x = the row's chunk partials in chunk order.  mode 0: HComputationReducer;
// 1: PPCHComputationReducer (+ optional L1 normalisation); 2: WComputationMapper (infinities clamped).  64 / L rows per wave;
// the sums over a row's columns are butterflies over its L lanes.
__global__ void __launch_bounds__(256)
k_rf_update(int32_t n_waves, int32_t K, const int32_t* __restrict__ rwave, const RfSeg* __restrict__ seg, const RfSeg* __restrict__ segC,
            const int32_t* __restrict__ chunkptr, const double* __restrict__ part, const double* __restrict__ M, const double* __restrict__ C_,
            int mode, int normalize, double* __restrict__ out) {
    const double eps = 1e-12;   // MatrixComputationJob.java:41
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int32_t w = blockIdx.x * wpb + (threadIdx.x >> 6); w < n_waves; w += gridDim.x * wpb) {
        const int32_t c = rf_find(rwave, K, w);
        const RfSeg S = seg[c];
        const int32_t k = S.k, L = S.L;
        const int32_t rl = (w - rwave[c]) * (64 / L) + lane / L, col = lane % L;
        const bool row_ok = rl < S.nrows;
        const int32_t r = S.row0 + (row_ok ? rl : 0);
        const double* __restrict__ m = M + S.moff + (int64_t)(row_ok ? rl : 0) * k;
        const double* __restrict__ C = C_ + segC[c].goff;
        const int32_t ch0 = chunkptr[r], ch1 = chunkptr[r + 1];
        double y[RF_MAX_K / 64], x[RF_MAX_K / 64], mv[RF_MAX_K / 64];
        double d = 0.0, e = 0.0;
#pragma unroll
        for (int q = 0; q < RF_MAX_K / 64; q++) {
            const int cc = col + 64 * q;
            y[q] = 0.0; x[q] = 0.0; mv[q] = 0.0;
            if (row_ok && cc < k) {
                double s = 0.0;
                for (int a = 0; a < k; a++) s += C[(int64_t)cc * k + a] * m[a];
                y[q] = s;
                double xs = 0.0;
                for (int32_t ch = ch0; ch < ch1; ch++) xs += part[S.poff + (int64_t)(ch - S.chunk0) * k + cc];
                x[q] = xs;
                mv[q] = m[cc];
                d += mv[q] * y[q];
                e += mv[q] * x[q];
            }
        }
        if (mode == 1)
            for (int o = L >> 1; o > 0; o >>= 1) { d += __shfl_xor(d, o, 64); e += __shfl_xor(e, o, 64); }
        double res[RF_MAX_K / 64], l1 = 0.0;
#pragma unroll
        for (int q = 0; q < RF_MAX_K / 64; q++) {
            const int cc = col + 64 * q;
            res[q] = 0.0;
            if (row_ok && cc < k) {
                double xx = x[q], yy = y[q];
                if (mode == 1) { xx = rf_clampinf(xx + d); yy = rf_clampinf(yy + e); }
                else if (mode == 2) { xx = rf_clampinf(xx); yy = rf_clampinf(yy); }
                res[q] = mv[q] * (xx / (yy + eps));
                l1 += fabs(res[q]);
            }
        }
        if (normalize)
            for (int o = L >> 1; o > 0; o >>= 1) l1 += __shfl_xor(l1, o, 64);
#pragma unroll
        for (int q = 0; q < RF_MAX_K / 64; q++) {
            const int cc = col + 64 * q;
            if (row_ok && cc < k) out[S.moff + (int64_t)rl * k + cc] = normalize ? res[q] / l1 : res[q];
        }
    }
}

// FindSubClusterMapper.java:53, 76: cluster = parent * stride + first index of the largest value (-1 if none exceeds -infinity)
__global__ void k_rf_assign(int32_t n_rows, const int32_t* __restrict__ user_raw, const int32_t* __restrict__ user_cl, const RfSeg* __restrict__ seg,
                            const double* __restrict__ H, int32_t stride, int32_t n_counts, int32_t* __restrict__ user, int32_t* __restrict__ cluster,
                            int32_t* __restrict__ count, int32_t* __restrict__ collisions, int* __restrict__ err) {
    for (int32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n_rows; g += gridDim.x * blockDim.x) {
        const int32_t c = user_cl[g];
        const RfSeg S = seg[c];
        const double* __restrict__ h = H + S.moff + (int64_t)(g - S.row0) * S.k;
        int32_t best = -1;
        double mx = -INFINITY;
        for (int32_t j = 0; j < S.k; j++) {
            const double v = h[j];
            if (v > mx) { mx = v; best = j; }
        }
        const int64_t id = best < 0 ? -1 : (int64_t)c * stride + best;
        user[g] = user_raw[g];
        cluster[g] = (int32_t)id;
        if (id < 0 || id >= n_counts) atomicOr(err, 1);
        else atomicAdd(&count[id], 1);
        if (best >= stride) atomicAdd(collisions, 1);
    }
}

inline int pow2_lanes(int k) {
    int L = 1;
    while (L < k && L < 64) L <<= 1;
    return L;
}

}  // namespace

// ---------------------------------------------------------------- SubClusterMappingJob
void build_submap(Context* ctx, const fy_ratings* R, int32_t K, int64_t n_map, const int32_t* map_user, const int32_t* map_cluster, SubMap& P) {
    if (K <= 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "Invalid number of clusters (%d)", K);      // RMRecommenderDriver.java:302-305
    if (n_map < 0 || (n_map > 0 && (!map_user || !map_cluster))) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "the clustering map is NULL or n_map < 0");
    if (n_map > INT32_MAX) FY_FAIL(FY_ERR_UNSUPPORTED, "more than 2^31 - 1 map entries");
    hipStream_t s = ctx->stream;
    int32_t max_map = -1;
    for (int64_t t = 0; t < n_map; t++) {
        if (map_user[t] < 0) FY_FAIL(FY_ERR_NEGATIVE_ID, "clustering map entry %lld: user id %d is negative", (long long)t, map_user[t]);
        max_map = std::max(max_map, map_user[t]);
    }
    if (std::max(max_map, R->max_user) == INT32_MAX) FY_FAIL(FY_ERR_UNSUPPORTED, "user id 2^31 - 1");
    const int32_t nT = std::max(max_map, R->max_user) + 1;
    const int64_t I64 = (int64_t)R->max_item + 1;       // (item id 2^31 - 1: the sum has no int32 value; refused by the bound below)
    if ((int64_t)K * std::max<int64_t>(I64, 1) + 1 > (int64_t)INT32_MAX) FY_FAIL(FY_ERR_UNSUPPORTED, "numberOfClusters x (largest item id + 1) exceeds 2^31");
    const int32_t I = (int32_t)I64;
    P.ctx = ctx; P.K = K; P.n_tab = nT; P.I = I;
    P.launches = 0;
    const int64_t n_in = R->nnz;
    const size_t nT1 = (size_t)std::max(nT, 1);

    // ---- users: the map's entries (InverseMapper over the `clustering` file); a later entry of one user replaces the earlier
    DevBuf<int32_t> d_mu(ctx, (size_t)std::max<int64_t>(1, n_map)), d_mc(ctx, (size_t)std::max<int64_t>(1, n_map)), last(ctx, nT1), n_members(ctx, 1);
    DevBuf<uint64_t> keys(ctx, nT1), keys_s(ctx, nT1);
    DevBuf<int> err(ctx, 1);
    SyncOnUnwind guard(s);
    h2d(ctx, d_mu.get(), map_user, (size_t)n_map);
    h2d(ctx, d_mc.get(), map_cluster, (size_t)n_map);
    FY_HIP(hipMemsetAsync(last.get(), 0xFF, nT1 * sizeof(int32_t), s));
    err.zero();
    n_members.zero();
    P.cl_of_raw.alloc(ctx, nT1);
    P.row_of_raw.alloc(ctx, nT1);
    FY_HIP(hipMemsetAsync(P.row_of_raw.get(), 0xFF, nT1 * sizeof(int32_t), s));
    if (n_map) {
        k_rf_last_entry<<<rf_grid(n_map), 256, 0, s>>>(n_map, d_mu.get(), last.get());
        FY_KERNEL_CHECK();
        P.launches++;
    }
    int32_t nU = 0;
    if (nT > 0) {
        k_rf_cluster_of_raw<<<rf_grid(nT), 256, 0, s>>>(nT, last.get(), d_mc.get(), K, P.cl_of_raw.get(), keys.get(), n_members.get(), err.get());
        FY_KERNEL_CHECK();
        sort_keys_u64(ctx, keys.get(), keys_s.get(), (size_t)nT, 64);
        P.launches += 2;
        nU = fetch(ctx, n_members.get());
        if (fetch(ctx, err.get())) FY_FAIL(FY_ERR_CLUSTER_RANGE, "a user of the clustering map is in a cluster outside [0, %d)", K);
    }
    P.n_users = nU;
    P.user_raw.alloc(ctx, (size_t)std::max(nU, 1));
    P.user_cl.alloc(ctx, (size_t)std::max(nU, 1));
    P.d_ustart.alloc(ctx, (size_t)K + 1);
    if (nU) {
        k_rf_user_rows<<<rf_grid(nU), 256, 0, s>>>(nU, keys_s.get(), P.user_raw.get(), P.user_cl.get(), P.row_of_raw.get());
        FY_KERNEL_CHECK();
        P.launches++;
    }
    k_rf_segptr<<<rf_grid((int64_t)K + 1), 256, 0, s>>>(K, nU, keys_s.get(), P.d_ustart.get());
    FY_KERNEL_CHECK();
    P.launches++;

    // ---- items: K x I presence words, prefix sums give the new ids (ascending raw id inside a cluster)
    const int64_t KI = (int64_t)K * I;
    DevBuf<int32_t> pres(ctx, (size_t)KI + 1);
    P.ipos.alloc(ctx, (size_t)KI + 1);
    pres.zero();
    if (n_in && I > 0) {
        k_rf_item_presence<<<rf_grid(n_in), 256, 0, s>>>(n_in, R->user.get(), R->item.get(), R->score.get(), nT, P.cl_of_raw.get(), K, I, pres.get(), err.get());
        FY_KERNEL_CHECK();
        P.launches++;
    }
    exclusive_scan_i32(ctx, pres.get(), P.ipos.get(), (size_t)KI + 1);
    P.launches++;
    const int32_t nI = fetch(ctx, P.ipos.get() + KI);
    if (fetch(ctx, err.get()) & 2) FY_FAIL(FY_ERR_NEGATIVE_ID, "a rating with score > 0 has a negative user or item id");
    P.n_items = nI;
    P.item_raw.alloc(ctx, (size_t)std::max(nI, 1));
    P.item_cl.alloc(ctx, (size_t)std::max(nI, 1));
    P.d_istart.alloc(ctx, (size_t)K + 1);
    if (KI > 0) {
        k_rf_item_rows<<<rf_grid(KI), 256, 0, s>>>(K, I, P.ipos.get(), P.item_raw.get(), P.item_cl.get(), P.d_istart.get());
        FY_KERNEL_CHECK();
        P.launches++;
    } else {
        FY_HIP(hipMemsetAsync(P.d_istart.get(), 0, ((size_t)K + 1) * sizeof(int32_t), s));
    }
    P.ustart.assign((size_t)K + 1, 0);
    P.istart.assign((size_t)K + 1, 0);
    d2h(ctx, P.ustart.data(), P.d_ustart.get(), (size_t)K + 1);
    d2h(ctx, P.istart.data(), P.d_istart.get(), (size_t)K + 1);

    // ---- the kept ratings, remapped: cluster-major CSR (by user row) and CSC (by item row), one sort each
    const size_t n1 = (size_t)std::max<int64_t>(1, n_in);
    DevBuf<uint64_t> ku(ctx, n1), ki(ctx, n1);
    DevBuf<unsigned long long> kept(ctx, 1);
    kept.zero();
    P.ku.alloc(ctx, n1); P.ki.alloc(ctx, n1); P.vu.alloc(ctx, n1); P.vi.alloc(ctx, n1);
    if (n_in) {
        k_rf_keys<<<rf_grid(n_in), 256, 0, s>>>(n_in, R->user.get(), R->item.get(), R->score.get(), nT, P.cl_of_raw.get(), P.row_of_raw.get(), I,
                                               P.ipos.get(), ku.get(), ki.get(), kept.get());
        FY_KERNEL_CHECK();
        sort_pairs_u64_f32(ctx, ku.get(), P.ku.get(), const_cast<float*>(R->score.get()), P.vu.get(), (size_t)n_in, 64);
        sort_pairs_u64_f32(ctx, ki.get(), P.ki.get(), const_cast<float*>(R->score.get()), P.vi.get(), (size_t)n_in, 64);
        P.launches += 3;
    }
    P.nnz = (int64_t)fetch(ctx, kept.get());      // (also drains the stream: ustart / istart are on the host)
    P.uptr.alloc(ctx, (size_t)nU + 1);
    P.iptr.alloc(ctx, (size_t)nI + 1);
    k_rf_segptr<<<rf_grid((int64_t)nU + 1), 256, 0, s>>>(nU, P.nnz, P.ku.get(), P.uptr.get());
    FY_KERNEL_CHECK();
    k_rf_segptr<<<rf_grid((int64_t)nI + 1), 256, 0, s>>>(nI, P.nnz, P.ki.get(), P.iptr.get());
    FY_KERNEL_CHECK();
    P.launches += 2;
    sync(ctx);
}

// ---------------------------------------------------------------- fy_cluster_refine
namespace {

struct Side {
    std::vector<RfSeg> seg;
    std::vector<int32_t> swave, rwave, gblock;      // K + 1 each
    DevBuf<RfSeg> d_seg;
    DevBuf<int32_t> d_swave, d_rwave, d_gblock, chunkptr, chunk_row;
    int32_t n_chunks = 0;
    int64_t m_total = 0, p_total = 0, g_total = 0, gp_total = 0;
};

void make_side(Context* ctx, int32_t K, const std::vector<int32_t>& start, const std::vector<int32_t>& kc, int32_t n_rows, const int32_t* rowptr,
               Side& sd, int64_t& launches) {
    hipStream_t s = ctx->stream;
    DevBuf<int32_t> cnt(ctx, (size_t)n_rows + 1);
    sd.chunkptr.alloc(ctx, (size_t)n_rows + 1);
    k_rf_chunk_counts<<<rf_grid((int64_t)n_rows + 1), 256, 0, s>>>(n_rows, rowptr, cnt.get());
    FY_KERNEL_CHECK();
    exclusive_scan_i32(ctx, cnt.get(), sd.chunkptr.get(), (size_t)n_rows + 1);
    launches += 2;
    std::vector<int32_t> cstart((size_t)K + 1);
    gather_to_host_i32(ctx, sd.chunkptr.get(), start, cstart.data());
    launches++;
    sd.n_chunks = cstart[(size_t)K];
    sd.chunk_row.alloc(ctx, (size_t)std::max(1, sd.n_chunks));
    if (n_rows) {
        k_rf_chunk_rows<<<rf_grid(n_rows), 256, 0, s>>>(n_rows, sd.chunkptr.get(), sd.chunk_row.get());
        FY_KERNEL_CHECK();
        launches++;
    }
    sd.seg.assign((size_t)K, RfSeg{});
    sd.swave.assign((size_t)K + 1, 0);
    sd.rwave.assign((size_t)K + 1, 0);
    sd.gblock.assign((size_t)K + 1, 0);
    int64_t sw = 0, rw = 0, gb = 0;
    for (int32_t c = 0; c < K; c++) {
        RfSeg& S = sd.seg[(size_t)c];
        S.row0 = start[(size_t)c];
        S.nrows = start[(size_t)c + 1] - start[(size_t)c];
        S.k = kc[(size_t)c];
        S.L = pow2_lanes(std::max(1, S.k));
        S.chunk0 = cstart[(size_t)c];
        S.nchunks = cstart[(size_t)c + 1] - cstart[(size_t)c];
        S.gram_rows = (int32_t)std::max<int64_t>(RF_GRAM_ROWS, ceil_div(S.nrows, RF_GRAM_BLOCKS));
        S.gram_nb = S.k > 0 ? (int32_t)ceil_div(S.nrows, S.gram_rows) : 0;
        S.moff = sd.m_total; S.poff = sd.p_total; S.goff = sd.g_total; S.gpoff = sd.gp_total;
        sd.m_total += (int64_t)S.nrows * S.k;
        sd.p_total += (int64_t)S.nchunks * S.k;
        sd.g_total += (int64_t)S.k * S.k;
        sd.gp_total += (int64_t)S.gram_nb * S.k * S.k;
        const int per = 64 / S.L;
        sw += S.k > 0 ? ceil_div(S.nchunks, per) : 0;
        rw += S.k > 0 ? ceil_div(S.nrows, per) : 0;
        gb += S.gram_nb;
        if (sw > INT32_MAX || rw > INT32_MAX || gb > INT32_MAX) FY_FAIL(FY_ERR_UNSUPPORTED, "the refinement's launch tables exceed 2^31 waves");
        sd.swave[(size_t)c + 1] = (int32_t)sw;
        sd.rwave[(size_t)c + 1] = (int32_t)rw;
        sd.gblock[(size_t)c + 1] = (int32_t)gb;
    }
    sd.d_seg.alloc(ctx, (size_t)K);
    sd.d_swave.alloc(ctx, (size_t)K + 1);
    sd.d_rwave.alloc(ctx, (size_t)K + 1);
    sd.d_gblock.alloc(ctx, (size_t)K + 1);
    h2d(ctx, sd.d_seg.get(), sd.seg.data(), (size_t)K);
    h2d(ctx, sd.d_swave.get(), sd.swave.data(), (size_t)K + 1);
    h2d(ctx, sd.d_rwave.get(), sd.rwave.data(), (size_t)K + 1);
    h2d(ctx, sd.d_gblock.get(), sd.gblock.data(), (size_t)K + 1);
}

}  // namespace

fy_refined* cluster_refine(Context* ctx, const fy_refine_params* prm, const fy_ratings* R, int64_t n_map, const int32_t* map_user,
                           const int32_t* map_cluster, const double* H0, const double* W0) {
    const int32_t K = prm->number_of_clusters, ups = prm->users_per_sub_cluster;
    hipStream_t s = ctx->stream;
    std::unique_ptr<fy_refined> res(new fy_refined);
    res->ctx = ctx;
    EventTimer t_total(ctx), t_map(ctx), t_iter(ctx), t_assign(ctx);
    const size_t sp_total = t_total.begin();
    const size_t sp_map = t_map.begin();
    SubMap P;
    build_submap(ctx, R, K, n_map, map_user, map_cluster, P);
    int64_t launches = P.launches;
    const int32_t nU = P.n_users, nI = P.n_items;
    // numberOfClusters of every sub-run (RMRecommenderDriver.java:239)
    std::vector<int32_t>& kc = res->k;
    kc.assign((size_t)K, 0);
    res->users_in_cluster.assign((size_t)K, 0);
    res->items_in_cluster.assign((size_t)K, 0);
    for (int32_t c = 0; c < K; c++) {
        const int32_t n = P.ustart[(size_t)c + 1] - P.ustart[(size_t)c];
        res->users_in_cluster[(size_t)c] = n;
        res->items_in_cluster[(size_t)c] = P.istart[(size_t)c + 1] - P.istart[(size_t)c];
        kc[(size_t)c] = (int32_t)ceil_div(n, ups);
        if (kc[(size_t)c] > RF_MAX_K)
            FY_FAIL(FY_ERR_UNSUPPORTED, "parent cluster %d: %d users / usersPerSubCluster %d = %d sub-clusters exceed the kernel limit %d", c, n, ups,
                    kc[(size_t)c], RF_MAX_K);
    }
    // a member without a kept rating (PPCHComputationReducer.java:50-57 / WComputationMapper.java:93-96 of the sub-run)
    if (prm->number_of_iterations > 0) {
        DevBuf<int32_t> empty(ctx, 2);
        FY_HIP(hipMemsetAsync(empty.get(), 0x7F, 2 * sizeof(int32_t), s));
        if (nU) k_rf_first_empty<<<rf_grid(nU), 256, 0, s>>>(nU, P.uptr.get(), P.user_cl.get(), P.d_ustart.get(), empty.get());
        FY_KERNEL_CHECK();
        if (nI) k_rf_first_empty<<<rf_grid(nI), 256, 0, s>>>(nI, P.iptr.get(), P.item_cl.get(), P.d_ustart.get(), empty.get() + 1);
        FY_KERNEL_CHECK();
        launches += 2;
        int32_t he[2];
        d2h(ctx, he, empty.get(), 2);
        sync(ctx);
        if (he[0] < nU) {
            const int32_t raw = fetch(ctx, P.user_raw.get() + he[0]), c = fetch(ctx, P.user_cl.get() + he[0]);
            FY_FAIL(FY_ERR_INVALID_ARGUMENT, "User %d has not rated any item (parent cluster %d)", raw, c);
        }
        if (he[1] < nI) {
            const int32_t raw = fetch(ctx, P.item_raw.get() + he[1]), c = fetch(ctx, P.item_cl.get() + he[1]);
            FY_FAIL(FY_ERR_INVALID_ARGUMENT, "Item %d has not been rated by anybody (parent cluster %d)", raw, c);
        }
    }
    Side U, V;
    SyncOnUnwind guard(s);      // (behind U / V: their host tables are sources of queued uploads)
    make_side(ctx, K, P.ustart, kc, nU, P.uptr.get(), U, launches);
    make_side(ctx, K, P.istart, kc, nI, P.iptr.get(), V, launches);
    t_map.end(sp_map);

    const size_t hN = (size_t)U.m_total, wN = (size_t)V.m_total;
    DevBuf<double> H2(ctx, std::max<size_t>(1, hN)), W2(ctx, std::max<size_t>(1, wN));
    DevBuf<double> C(ctx, (size_t)std::max<int64_t>(1, U.g_total)), gpart(ctx, (size_t)std::max<int64_t>(1, std::max(U.gp_total, V.gp_total)));
    DevBuf<double> spart(ctx, (size_t)std::max<int64_t>(1, std::max(U.p_total, V.p_total)));
    res->H.alloc(ctx, std::max<size_t>(1, hN));
    res->W.alloc(ctx, std::max<size_t>(1, wN));
    res->h_size = (int64_t)hN;
    res->w_size = (int64_t)wN;
    const int32_t rwU = U.rwave[(size_t)K], rwV = V.rwave[(size_t)K], swU = U.swave[(size_t)K], swV = V.swave[(size_t)K];
    const int32_t gbU = U.gblock[(size_t)K], gbV = V.gblock[(size_t)K];
    if (H0 && W0) {
        h2d(ctx, res->H.get(), H0, hN);
        h2d(ctx, res->W.get(), W0, wN);
    } else {
        if (rwU) k_rf_init<<<rf_grid((int64_t)rwU * 64), 256, 0, s>>>(rwU, K, U.d_rwave.get(), U.d_seg.get(), prm->seed, 0u, res->H.get());
        FY_KERNEL_CHECK();
        if (rwV) k_rf_init<<<rf_grid((int64_t)rwV * 64), 256, 0, s>>>(rwV, K, V.d_rwave.get(), V.d_seg.get(), prm->seed, 1u, res->W.get());
        FY_KERNEL_CHECK();
        launches += 2;
    }
    double* h = res->H.get();
    double* w = res->W.get();
    double* h2 = H2.get();
    double* w2 = W2.get();
    const int f = prm->normalization_frequency;
    const size_t sp_iter = t_iter.begin();
    const bool work = rwU > 0 && rwV > 0 && swU > 0 && swV > 0 && gbU > 0 && gbV > 0;
    for (int32_t it = 1; work && it <= prm->number_of_iterations; it++) {
        // H2 from (H, W)
        k_rf_spmm<<<rf_grid((int64_t)swU * 64), 256, 0, s>>>(swU, K, U.d_swave.get(), U.d_seg.get(), V.d_seg.get(), U.chunk_row.get(), U.chunkptr.get(),
                                                            P.uptr.get(), P.ku.get(), P.vu.get(), w, spart.get());
        FY_KERNEL_CHECK();
        k_rf_gram_partial<<<gbV, 256, 0, s>>>(K, V.d_gblock.get(), V.d_seg.get(), w, gpart.get());
        FY_KERNEL_CHECK();
        k_rf_gram_sum<<<dim3((unsigned)K, 4), 256, 0, s>>>(V.d_seg.get(), gpart.get(), C.get());
        FY_KERNEL_CHECK();
        const int normalize = prm->ppc && f != 0 && (it % f == 0);   // Java %: f = -1 (the key left unset) normalises every iteration
        k_rf_update<<<rf_grid((int64_t)rwU * 64), 256, 0, s>>>(rwU, K, U.d_rwave.get(), U.d_seg.get(), V.d_seg.get(), U.chunkptr.get(), spart.get(), h,
                                                              C.get(), prm->ppc ? 1 : 0, normalize, h2);
        FY_KERNEL_CHECK();
        // W2 from the same (H, W)
        k_rf_spmm<<<rf_grid((int64_t)swV * 64), 256, 0, s>>>(swV, K, V.d_swave.get(), V.d_seg.get(), U.d_seg.get(), V.chunk_row.get(), V.chunkptr.get(),
                                                            P.iptr.get(), P.ki.get(), P.vi.get(), h, spart.get());
        FY_KERNEL_CHECK();
        k_rf_gram_partial<<<gbU, 256, 0, s>>>(K, U.d_gblock.get(), U.d_seg.get(), h, gpart.get());
        FY_KERNEL_CHECK();
        k_rf_gram_sum<<<dim3((unsigned)K, 4), 256, 0, s>>>(U.d_seg.get(), gpart.get(), C.get());
        FY_KERNEL_CHECK();
        k_rf_update<<<rf_grid((int64_t)rwV * 64), 256, 0, s>>>(rwV, K, V.d_rwave.get(), V.d_seg.get(), U.d_seg.get(), V.chunkptr.get(), spart.get(), w,
                                                              C.get(), 2, 0, w2);
        FY_KERNEL_CHECK();
        launches += 8;
        std::swap(h, h2);
        std::swap(w, w2);
    }
    if (h != res->H.get()) { std::swap(res->H, H2); std::swap(res->W, W2); }
    t_iter.end(sp_iter);

    // ---- ClusterAssignmentJob(true): cluster = parent * ceil(numberOfUsers / numberOfClusters) + argmax
    const size_t sp_assign = t_assign.begin();
    const int64_t stride = ceil_div(prm->number_of_users, K);
    int64_t n_counts = stride * K;
    for (int32_t c = 0; c < K; c++)
        if (kc[(size_t)c] > 0) n_counts = std::max<int64_t>(n_counts, c * stride + kc[(size_t)c]);
    if (n_counts > INT32_MAX) FY_FAIL(FY_ERR_UNSUPPORTED, "cluster ids exceed 2^31");
    res->stride = (int32_t)stride;
    res->user.assign((size_t)nU, 0);
    res->cluster.assign((size_t)nU, 0);
    res->count.assign((size_t)n_counts, 0);
    DevBuf<int32_t> d_user(ctx, (size_t)std::max(1, nU)), d_cluster(ctx, (size_t)std::max(1, nU)), d_count(ctx, (size_t)std::max<int64_t>(1, n_counts)), coll(ctx, 1);
    DevBuf<int> err(ctx, 1);
    d_count.zero();
    coll.zero();
    err.zero();
    if (nU) {
        k_rf_assign<<<rf_grid(nU), 256, 0, s>>>(nU, P.user_raw.get(), P.user_cl.get(), U.d_seg.get(), res->H.get(), (int32_t)stride, (int32_t)n_counts,
                                               d_user.get(), d_cluster.get(), d_count.get(), coll.get(), err.get());
        FY_KERNEL_CHECK();
        launches++;
    }
    d2h(ctx, res->user.data(), d_user.get(), (size_t)nU);
    d2h(ctx, res->cluster.data(), d_cluster.get(), (size_t)nU);
    d2h(ctx, res->count.data(), d_count.get(), (size_t)n_counts);
    int32_t hcoll = 0;
    int herr = 0;
    d2h(ctx, &hcoll, coll.get(), 1);
    d2h(ctx, &herr, err.get(), 1);
    t_assign.end(sp_assign);
    t_total.end(sp_total);
    sync(ctx);
    if (herr) FY_FAIL(FY_ERR_CLUSTER_RANGE, "a row of a refined H has no value above -infinity: its user has no cluster");
    fy_refine_stats& st = res->stats;
    st = fy_refine_stats{};
    st.ms_mappings = t_map.total_ms();
    st.ms_iterations = t_iter.total_ms();
    st.ms_assign = t_assign.total_ms();
    st.ms_total = t_total.total_ms();
    st.launches = launches;
    st.sum_users = nU;
    st.sum_items = nI;
    for (int32_t c = 0; c < K; c++) st.sum_k += kc[(size_t)c];
    st.nnz = P.nnz;
    st.collisions = hcoll;
    return res.release();
}

}  // namespace fy

// ---------------------------------------------------------------- C ABI
#define RF_TRY try {
#define RF_CATCH                                                           \
    }                                                                      \
    catch (const fy::Failure& f) { return f.code; }                        \
    catch (const std::bad_alloc&) {                                        \
        fy::set_error("host allocation failed");                           \
        return FY_ERR_OUT_OF_MEMORY;                                       \
    }                                                                      \
    catch (const std::exception& e) {                                      \
        fy::set_error("unexpected: %s", e.what());                         \
        return FY_ERR_HIP;                                                 \
    }                                                                      \
    return FY_OK;

struct fy_submap {
    fy::SubMap m;
};

extern "C" {

int fy_submap_create(fy_context* c, const fy_ratings* r, int32_t number_of_clusters, int64_t n_map, const int32_t* map_user,
                     const int32_t* map_cluster, fy_submap** out) {
    if (!out) { fy::set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (number_of_clusters <= 0) { fy::set_error("Invalid number of clusters (%d)", number_of_clusters); return FY_ERR_INVALID_ARGUMENT; }
    if (n_map < 0 || (n_map > 0 && (!map_user || !map_cluster))) { fy::set_error("the clustering map is NULL or n_map < 0"); return FY_ERR_INVALID_ARGUMENT; }
    if (!c || !r) { fy::set_error("context or ratings is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->ctx != &c->c) { fy::set_error("ratings belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    RF_TRY
    FY_HIP(hipSetDevice(c->c.device));
    std::unique_ptr<fy_submap> m(new fy_submap);
    fy::build_submap(&c->c, r, number_of_clusters, n_map, map_user, map_cluster, m->m);
    *out = m.release();
    RF_CATCH
}

int64_t fy_submap_n_users(const fy_submap* m) { return m ? m->m.n_users : 0; }
int64_t fy_submap_n_items(const fy_submap* m) { return m ? m->m.n_items : 0; }
int64_t fy_submap_nnz(const fy_submap* m) { return m ? m->m.nnz : 0; }

int fy_submap_counts(const fy_submap* m, int32_t* users_in_cluster, int32_t* items_in_cluster) {
    if (!m || !users_in_cluster || !items_in_cluster) { fy::set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    for (int32_t c = 0; c < m->m.K; c++) {
        users_in_cluster[c] = m->m.ustart[(size_t)c + 1] - m->m.ustart[(size_t)c];
        items_in_cluster[c] = m->m.istart[(size_t)c + 1] - m->m.istart[(size_t)c];
    }
    return FY_OK;
}

static void rf_new_ids(const std::vector<int32_t>& start, int64_t n, const int32_t* cluster, int32_t* new_id) {
    for (int64_t g = 0; g < n; g++) new_id[g] = (int32_t)(g - start[(size_t)cluster[g]]) + 1;
}

int fy_submap_users(fy_submap* m, int32_t* raw_user, int32_t* cluster, int32_t* new_id) {
    if (!m || !raw_user || !cluster || !new_id) { fy::set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    RF_TRY
    fy::Context* ctx = m->m.ctx;
    FY_HIP(hipSetDevice(ctx->device));
    fy::d2h(ctx, raw_user, m->m.user_raw.get(), (size_t)m->m.n_users);
    fy::d2h(ctx, cluster, m->m.user_cl.get(), (size_t)m->m.n_users);
    fy::sync(ctx);
    rf_new_ids(m->m.ustart, m->m.n_users, cluster, new_id);
    RF_CATCH
}

int fy_submap_items(fy_submap* m, int32_t* raw_item, int32_t* cluster, int32_t* new_id) {
    if (!m || !raw_item || !cluster || !new_id) { fy::set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    RF_TRY
    fy::Context* ctx = m->m.ctx;
    FY_HIP(hipSetDevice(ctx->device));
    fy::d2h(ctx, raw_item, m->m.item_raw.get(), (size_t)m->m.n_items);
    fy::d2h(ctx, cluster, m->m.item_cl.get(), (size_t)m->m.n_items);
    fy::sync(ctx);
    rf_new_ids(m->m.istart, m->m.n_items, cluster, new_id);
    RF_CATCH
}

int fy_submap_matrix(fy_submap* m, int by_item, int32_t* rowptr, int32_t* col, float* value) {
    if (!m || !rowptr || (m->m.nnz > 0 && (!col || !value))) { fy::set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    RF_TRY
    fy::Context* ctx = m->m.ctx;
    FY_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)m->m.nnz;
    std::vector<uint64_t> keys(n);
    fy::d2h(ctx, rowptr, (by_item ? m->m.iptr : m->m.uptr).get(), (size_t)(by_item ? m->m.n_items : m->m.n_users) + 1);
    fy::d2h(ctx, keys.data(), (by_item ? m->m.ki : m->m.ku).get(), n);
    fy::d2h(ctx, value, (by_item ? m->m.vi : m->m.vu).get(), n);
    fy::sync(ctx);
    for (size_t t = 0; t < n; t++) col[t] = (int32_t)(uint32_t)keys[t];
    RF_CATCH
}

void fy_submap_destroy(fy_submap* m) {
    if (!m) return;
    if (m->m.ctx) { (void)hipSetDevice(m->m.ctx->device); (void)hipStreamSynchronize(m->m.ctx->stream); }
    delete m;
}

int fy_cluster_refine(fy_context* c, const fy_refine_params* p, const fy_ratings* r, int64_t n_map, const int32_t* map_user,
                      const int32_t* map_cluster, const double* H0, const double* W0, fy_refined** out) {
    if (!out) { fy::set_error("out is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!p) { fy::set_error("params is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (p->number_of_clusters <= 0) { fy::set_error("Invalid number of clusters (%d)", p->number_of_clusters); return FY_ERR_INVALID_ARGUMENT; }
    if (p->users_per_sub_cluster <= 0) { fy::set_error("usersPerSubCluster must be > 0 (%d)", p->users_per_sub_cluster); return FY_ERR_INVALID_ARGUMENT; }
    if (p->number_of_users <= 0 || p->number_of_iterations < 0) { fy::set_error("numberOfUsers must be > 0 and numberOfIterations >= 0"); return FY_ERR_INVALID_ARGUMENT; }
    if (n_map < 0 || (n_map > 0 && (!map_user || !map_cluster))) { fy::set_error("the clustering map is NULL or n_map < 0"); return FY_ERR_INVALID_ARGUMENT; }
    if ((H0 == nullptr) != (W0 == nullptr)) { fy::set_error("H0 and W0 must be given together or both be NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (!c || !r) { fy::set_error("context or ratings is NULL"); return FY_ERR_INVALID_ARGUMENT; }
    if (r->ctx != &c->c) { fy::set_error("ratings belong to another context"); return FY_ERR_INVALID_ARGUMENT; }
    RF_TRY
    FY_HIP(hipSetDevice(c->c.device));
    *out = fy::cluster_refine(&c->c, p, r, n_map, map_user, map_cluster, H0, W0);
    RF_CATCH
}

int64_t fy_refined_n_users(const fy_refined* r) { return r ? (int64_t)r->user.size() : 0; }
int64_t fy_refined_n_counts(const fy_refined* r) { return r ? (int64_t)r->count.size() : 0; }
int64_t fy_refined_h_size(const fy_refined* r) { return r ? r->h_size : 0; }
int64_t fy_refined_w_size(const fy_refined* r) { return r ? r->w_size : 0; }

int fy_refined_clustering(const fy_refined* r, int32_t* user, int32_t* cluster, int32_t* count) {
    if (!r || (!r->user.empty() && (!user || !cluster)) || (!r->count.empty() && !count)) { fy::set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    if (!r->user.empty()) {
        memcpy(user, r->user.data(), r->user.size() * sizeof(int32_t));
        memcpy(cluster, r->cluster.data(), r->cluster.size() * sizeof(int32_t));
    }
    if (!r->count.empty()) memcpy(count, r->count.data(), r->count.size() * sizeof(int32_t));
    return FY_OK;
}

int fy_refined_layout(const fy_refined* r, int32_t* users_in_cluster, int32_t* items_in_cluster, int32_t* sub_clusters) {
    if (!r || !users_in_cluster || !items_in_cluster || !sub_clusters) { fy::set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    for (size_t c = 0; c < r->k.size(); c++) {
        users_in_cluster[c] = r->users_in_cluster[c];
        items_in_cluster[c] = r->items_in_cluster[c];
        sub_clusters[c] = r->k[c];
    }
    return FY_OK;
}

int fy_refined_factors(fy_refined* r, double* H, double* W) {
    if (!r || (r->h_size > 0 && !H) || (r->w_size > 0 && !W)) { fy::set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    RF_TRY
    FY_HIP(hipSetDevice(r->ctx->device));
    fy::d2h(r->ctx, H, r->H.get(), (size_t)r->h_size);
    fy::d2h(r->ctx, W, r->W.get(), (size_t)r->w_size);
    fy::sync(r->ctx);
    RF_CATCH
}

int fy_refined_stats(const fy_refined* r, fy_refine_stats* out) {
    if (!r || !out) { fy::set_error("NULL argument"); return FY_ERR_INVALID_ARGUMENT; }
    *out = r->stats;
    return FY_OK;
}

void fy_refined_free(fy_refined* r) {
    if (!r) return;
    if (r->ctx) { (void)hipSetDevice(r->ctx->device); (void)hipStreamSynchronize(r->ctx->stream); }
    delete r;
}

}  // extern "C"
