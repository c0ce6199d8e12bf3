// fy_foldin.hip -- fold-in: assign GIVEN profiles to clusters from the standing factors (fy_foldin_*).
//
// The standard fold-in of a factorisation: the item factors W of the last PPC / NMF run are held fixed and the reference's own H update
// (HComputationReducer.java:57-75 / PPCHComputationReducer.java:61-96) runs for the new rows alone; the cluster is the argmax
// (FindClusterMapper.java:37-45; with a refined level FindSubClusterMapper.java:46-76 on the parent's factors).  Work: sized by the
// request -- a gather of entries x k doubles plus iterations x k^2 flops per profile.
//   ingest     k_fi_keys, sort_pairs_u64_u32 (stable), k_fi_runs, exclusive_scan_i32, k_fi_rowptr, k_fi_scatter: the sequence of the
//              other profile calls with the factorisation's own rules -- an id outside [1, numberOfItems] is
//              dropped first, the last entry per item counts, a delete or a score that is not > 0 (k_nmf_keys) removes the item; the
//              composed rows are in ascending item id, the order of the factorisation's CSR rows
//   k_foldin   one wave per profile and level: x = sum a_i W[row_i][:] in the summation order of k_nmf_spmm_chunks + k_nmf_spmm_reduce,
//              `iterations` updates of h in registers through nmf_update_row (the row body of k_nmf_update), argmax by k_argmax_rows'
//              rule over the allowed columns
// All stores are plain vector stores, there are no floating-point atomics; the counters are a handful of wave-aggregated atomics.
// Known limit: at small k most lanes idle during the gather (the ordered sum forbids spreading the entries over lane groups).
#include <algorithm>
#include <limits>

#include "fy_foldin.hpp"
#include "fy_nmf_kernels.hpp"
#include "fy_prep.hpp"

namespace fy {
namespace {

enum { FC_OUT_OF_RANGE = 0, FC_SUPERSEDED, FC_REMOVED, FC_NONPOSITIVE, FC_EMPTY, FC_N };

inline int bits_for(int64_t v) {      // bits needed to hold the values 0 .. v
    int b = 1;
    while (b < 63 && (v >> b) != 0) b++;
    return b;
}

__device__ __forceinline__ void fi_count(unsigned long long* __restrict__ counters, int which, bool mine) {      // whole waves call it
    const unsigned long long b = __ballot(mine);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&counters[which], (unsigned long long)__popcll(b));
}

struct FoldIn {
    int32_t n, T;               // profiles and entries of this rank
    int32_t items;              // numberOfItems
    int cb;                     // bits of item id - 1
    const int32_t* start;       // n + 1, from 0
    const int32_t* item;
    const float* score;
    const uint8_t* remove;      // or nullptr
};

// key = profile << cb | (item id - 1); an id outside [1, items] gets the key of profile n: it sorts behind everything
__global__ void k_fi_keys(FoldIn A, uint64_t* __restrict__ keys, uint32_t* __restrict__ pos, unsigned long long* __restrict__ counters) {
    const int64_t t_up = ((int64_t)A.T + 63) & ~(int64_t)63;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < t_up; t += (int64_t)gridDim.x * blockDim.x) {
        bool outside = false;
        if (t < A.T) {
            const int32_t p = fy_lower_bound<true>(A.start, 0, A.n, (int32_t)t) - 1;
            const int32_t id = A.item[t];
            outside = id < 1 || id > A.items;
            keys[t] = outside ? ((uint64_t)(uint32_t)A.n << A.cb) : (((uint64_t)(uint32_t)p << A.cb) | (uint32_t)(id - 1));
            pos[t] = (uint32_t)t;
        }
        fi_count(counters, FC_OUT_OF_RANGE, outside);
    }
}

// keep[x] (x <= T; keep[T] = 0): sorted element x is the last of its key's run, no delete, and its score is > 0
__global__ void k_fi_runs(FoldIn A, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ spos, int32_t* __restrict__ keep,
                          unsigned long long* __restrict__ counters) {
    const int64_t t_up = ((int64_t)A.T + 1 + 63) & ~(int64_t)63;
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < t_up; x += (int64_t)gridDim.x * blockDim.x) {
        int kind = -1;      // 0 superseded, 1 a delete, 2 a score that is not > 0
        bool k = false;
        if (x < A.T) {
            const uint64_t key = skeys[x];
            if ((int32_t)(key >> A.cb) < A.n) {
                const bool last = x == A.T - 1 || skeys[x + 1] != key;
                const int32_t t = (int32_t)spos[x];
                if (!last) kind = 0;
                else if (A.remove && A.remove[t]) kind = 1;
                else if (!(A.score[t] > 0.0f)) kind = 2;
                else k = true;
            }
        }
        if (x <= A.T) keep[x] = k;
        fi_count(counters, FC_SUPERSEDED, kind == 0);
        fi_count(counters, FC_REMOVED, kind == 1);
        fi_count(counters, FC_NONPOSITIVE, kind == 2);
    }
}

// rowptr[p], p <= n: the place of the first kept element of profile p (place[T] = all kept elements)
__global__ void k_fi_rowptr(int32_t n, int32_t T, int cb, const uint64_t* __restrict__ skeys, const int32_t* __restrict__ place,
                            int32_t* __restrict__ rowptr, unsigned long long* __restrict__ counters) {
    const int64_t n_up = ((int64_t)n + 1 + 63) & ~(int64_t)63;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n_up; p += (int64_t)gridDim.x * blockDim.x) {
        bool empty = false;
        if (p <= n) {
            const int32_t a = place[fy_lower_bound(skeys, 0, T, (uint64_t)p << cb)];
            rowptr[p] = a;
            if (p < n) empty = place[fy_lower_bound(skeys, 0, T, (uint64_t)(p + 1) << cb)] == a;
        }
        fi_count(counters, FC_EMPTY, empty);
    }
}

__global__ void k_fi_scatter(FoldIn A, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ spos, const int32_t* __restrict__ keep,
                             const int32_t* __restrict__ place, int32_t* __restrict__ o_idx, float* __restrict__ o_val) {
    const uint64_t col_mask = ((uint64_t)1 << A.cb) - 1;
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < A.T; x += (int64_t)gridDim.x * blockDim.x) {
        if (!keep[x]) continue;
        const int32_t at = place[x];
        o_idx[at] = (int32_t)(skeys[x] & col_mask);
        o_val[at] = A.score[spos[x]];
    }
}

struct FoldArgs {
    int32_t n;
    const int32_t* rowptr;      // the composed profiles: n + 1
    const int32_t* idx;         // item id - 1, ascending inside a profile
    const float* val;
    const FoldBlock* blocks;
    const int32_t* block_of;    // n: the block of every profile (< 0: passed over); nullptr: block 0
    const double* h0;           // n x k of block 0, or nullptr: uniform 1 / k
    const int64_t* out_off;     // n: where the profile's factor row goes; nullptr: p * k of block 0
    int32_t iterations, first_iteration, ppc, f;
    double* out;
    int32_t* arg;               // n: first index of the strictly largest allowed value, -1: none exceeds -infinity
    int32_t* found;             // n: entries that have a row in the block
};

// the lanes of a wave exchange h through their LDS row: order the row's writes and reads
__device__ __forceinline__ void fold_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave per profile.  c0_in_lds: every profile runs on block 0 and its k <= 64: C is staged in LDS as k_nmf_update has it.
__global__ void __launch_bounds__(256) k_foldin(FoldArgs A, int c0_in_lds) {
    constexpr int Q = NMF_MAX_K / 64;
    __shared__ double shC[64 * 65];
    __shared__ double shH[4][NMF_MAX_K];
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (c0_in_lds) {
        const int32_t k0 = A.blocks[0].k;
        const double* __restrict__ C0 = A.blocks[0].C;
        for (int e = threadIdx.x; e < k0 * k0; e += blockDim.x) shC[(e / k0) * 65 + (e % k0)] = C0[e];
        __syncthreads();
    }
    double* hrow = shH[w];
    for (int32_t p = blockIdx.x * wpb + w; p < A.n; p += gridDim.x * wpb) {
        const int32_t b = A.block_of ? __builtin_amdgcn_readfirstlane(A.block_of[p]) : 0;
        if (b < 0) {
            if (lane == 0) { A.arg[p] = -1; A.found[p] = 0; }
            continue;
        }
        const FoldBlock B = A.blocks[b];
        const int32_t k = B.k;
        const double* __restrict__ C = c0_in_lds ? shC : B.C;
        const int ldc = c0_in_lds ? 65 : k;
        // ---- x = sum a_i W[row_i][:] over the entries with a row, in entry order: chunks of NMF_CHUNK summed from 0.0, then the chunk
        // sums added from 0.0 (k_nmf_spmm_chunks + k_nmf_spmm_reduce); up to four entries in flight
        double acc[Q], x[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) { acc[q] = 0.0; x[q] = 0.0; }
        int32_t in_chunk = 0, n_found = 0;
        const int32_t e0 = A.rowptr[p], e1 = A.rowptr[p + 1];
        for (int32_t base = e0; base < e1; base += 64) {
            const int32_t e = base + lane;
            int32_t row = -1;
            double a = 0.0;
            if (e < e1) {
                const int32_t id0 = A.idx[e];
                if (B.items) {
                    const int32_t lo = fy_lower_bound(B.items, 0, B.m, id0 + 1);
                    row = lo < B.m && B.items[lo] == id0 + 1 ? lo : -1;
                } else {
                    row = id0;      // the ingest kept only ids in [1, numberOfItems]
                }
                a = (double)A.val[e];
            }
            unsigned long long mask = __ballot(row >= 0);
            n_found += (int32_t)__popcll(mask);
            while (mask) {
                const int g = min(min(4, (int)__popcll(mask)), NMF_CHUNK - in_chunk);      // a group never crosses a chunk
                int j[4];
                j[0] = __ffsll((long long)mask) - 1;
#pragma unroll
                for (int u = 1; u < 4; u++) {
                    if (u < g) { mask &= mask - 1; j[u] = __ffsll((long long)mask) - 1; }
                    else j[u] = j[u - 1];      // a tail slot re-reads the last entry and is skipped below
                }
                mask &= mask - 1;
                double av[4];
                const double* bw[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    av[u] = __shfl(a, j[u], 64);
                    bw[u] = B.W + (int64_t)__shfl(row, j[u], 64) * k;
                }
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    const int c = lane + 64 * q;
                    if (c < k) {
                        const double v0 = bw[0][c], v1 = bw[1][c], v2 = bw[2][c], v3 = bw[3][c];
                        acc[q] += av[0] * v0;
                        if (1 < g) acc[q] += av[1] * v1;
                        if (2 < g) acc[q] += av[2] * v2;
                        if (3 < g) acc[q] += av[3] * v3;
                    }
                }
                in_chunk += g;
                if (in_chunk == NMF_CHUNK) {
#pragma unroll
                    for (int q = 0; q < Q; q++) { x[q] += acc[q]; acc[q] = 0.0; }
                    in_chunk = 0;
                }
            }
        }
        if (in_chunk > 0) {
#pragma unroll
            for (int q = 0; q < Q; q++) x[q] += acc[q];
        }
        // ---- the updates of h, in registers; the lanes read each other's columns through the wave's LDS row
        double h[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int c = lane + 64 * q;
            h[q] = c < k ? (A.h0 ? A.h0[(int64_t)p * k + c] : 1.0 / (double)k) : 0.0;
        }
        for (int32_t i = 0; i < A.iterations; i++) {
            const int32_t it = A.first_iteration + i;
            const int normalize = A.ppc && A.f != 0 && (it % A.f == 0);
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int c = lane + 64 * q;
                if (c < k) hrow[c] = h[q];
            }
            fold_wave_sync();
            double h2[Q];
            nmf_update_row(k, lane, hrow, x, C, ldc, A.ppc ? 1 : 0, normalize, h2);
            fold_wave_sync();
#pragma unroll
            for (int q = 0; q < Q; q++) h[q] = h2[q];
        }
        // ---- the factor row and its argmax over the allowed columns (k_argmax_rows: first index of the strictly largest value, NaN never wins)
        const int64_t off = A.out_off ? A.out_off[p] : (int64_t)p * k;
        int32_t best = -1;
        double mx = -INFINITY;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int c = lane + 64 * q;
            if (c < k) {
                A.out[off + c] = h[q];
                if ((!B.allowed || B.allowed[c]) && h[q] > mx) { mx = h[q]; best = c; }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double om = __shfl_xor(mx, o, 64);
            const int32_t ob = __shfl_xor(best, o, 64);
            if (ob >= 0 && (om > mx || (om == mx && (best < 0 || ob < best)))) { mx = om; best = ob; }
        }
        if (lane == 0) { A.arg[p] = best; A.found[p] = n_found; }
    }
}

void check_counts(const int32_t* count, int64_t n_count) {
    if (n_count < 0 || (n_count > 0 && !count)) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "count is NULL with n_count > 0, or n_count < 0");
}

// uploads the descriptors of every block the model holds
void publish_blocks(fy_foldin* F) {
    Context* ctx = F->ctx;
    std::vector<FoldBlock> hb((size_t)1 + F->n_parents);
    hb[0] = FoldBlock{F->W.get(), F->C.get(), nullptr, F->has_mask0 ? F->allowed0.get() : nullptr, F->prm.number_of_items, F->prm.number_of_clusters};
    for (int32_t c = 0; c < F->n_parents; c++)
        hb[(size_t)1 + c] = FoldBlock{F->W1.get() + F->w_off[c], F->C1.get() + F->c_off[c], F->items1.get() + F->i_off[c],
                                      F->has_mask1 ? F->allowed1.get() + F->a_off[c] : nullptr, F->m_c[c], F->k_c[c]};
    DevBuf<FoldBlock> d(ctx, hb.size());
    SyncOnUnwind drain(ctx->stream);
    h2d(ctx, d.get(), hb.data(), hb.size());
    sync(ctx);
    F->blocks = std::move(d);
}

}  // namespace

fy_foldin* foldin_create(Context* ctx, const fy_foldin_params* prm, const double* W, int location, const int32_t* count, int64_t n_count) {
    const int32_t m = prm->number_of_items, k = prm->number_of_clusters;
    std::unique_ptr<fy_foldin> F(new fy_foldin);
    F->ctx = ctx;
    F->prm = *prm;
    F->W.alloc(ctx, (size_t)m * k);
    F->C.alloc(ctx, (size_t)k * k);
    F->allowed0.alloc(ctx, (size_t)k);
    std::vector<uint8_t> ok((size_t)k, 0);
    F->has_mask0 = count != nullptr;
    for (int32_t c = 0; c < k && count; c++) ok[(size_t)c] = c < n_count && count[c] > 0;
    SyncOnUnwind drain(ctx->stream);
    if (location == FY_HOST) h2d(ctx, F->W.get(), W, (size_t)m * k);
    else d2d(ctx, F->W.get(), W, (size_t)m * k);
    h2d(ctx, F->allowed0.get(), ok.data(), (size_t)k);
    {
        DevBuf<double> part(ctx, (size_t)NMF_GRAM_BLOCKS * k * k);
        nmf_gram(ctx, m, k, F->W.get(), part.get(), F->C.get());      // bitwise the C of the factorisation's H half
    }
    sync(ctx);
    publish_blocks(F.get());
    return F.release();
}

void foldin_add_level(fy_foldin* F, int32_t n_parents, const int32_t* items_in_cluster, const int32_t* sub_clusters, const int32_t* item_raw,
                      const double* W_ragged, int32_t stride, const int32_t* count, int64_t n_count) {
    Context* ctx = F->ctx;
    // ---- refused on the host, before anything of the model changes
    if (F->n_parents) FY_FAIL(FY_ERR_STATE, "the model already holds a refined level");
    if (n_parents != F->prm.number_of_clusters)
        FY_FAIL(FY_ERR_INVALID_ARGUMENT, "n_parents is %d: the refined level has one block per top-level cluster (%d)", n_parents, F->prm.number_of_clusters);
    if (!items_in_cluster || !sub_clusters) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "items_in_cluster or sub_clusters is NULL");
    if (stride <= 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "stride must be > 0 (%d)", stride);
    check_counts(count, n_count);
    std::vector<int64_t> w_off((size_t)n_parents + 1, 0), c_off(w_off), i_off(w_off), a_off(w_off);
    for (int32_t c = 0; c < n_parents; c++) {
        const int32_t mc = items_in_cluster[c], kc = sub_clusters[c];
        if (mc < 0 || kc < 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "parent cluster %d: items_in_cluster / sub_clusters < 0", c);
        if (kc > NMF_MAX_K) FY_FAIL(FY_ERR_UNSUPPORTED, "parent cluster %d: %d sub-clusters exceed the kernel limit %d", c, kc, NMF_MAX_K);
        w_off[(size_t)c + 1] = w_off[c] + (int64_t)mc * kc;
        c_off[(size_t)c + 1] = c_off[c] + (int64_t)kc * kc;
        i_off[(size_t)c + 1] = i_off[c] + mc;
        a_off[(size_t)c + 1] = a_off[c] + kc;
    }
    if (i_off[n_parents] > 0 && !item_raw) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "item_raw is NULL");
    if (w_off[n_parents] > 0 && !W_ragged) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "W_ragged is NULL");
    for (int32_t c = 0; c < n_parents; c++)
        for (int64_t t = i_off[c] + 1; t < i_off[(size_t)c + 1]; t++)
            if (item_raw[t] <= item_raw[t - 1]) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "parent cluster %d: the item list is not ascending at position %lld", c, (long long)(t - i_off[c]));
    // ---- masks: a sub-cluster is allowed when it has resident users, a parent when any of its sub-clusters has
    std::vector<uint8_t> ok1((size_t)a_off[n_parents], 0), ok0((size_t)n_parents, 0);
    if (count) {
        for (int32_t c = 0; c < n_parents; c++)
            for (int32_t j = 0; j < sub_clusters[c]; j++) {
                const int64_t id = (int64_t)c * stride + j;
                const bool has = id < n_count && count[id] > 0;
                ok1[(size_t)(a_off[c] + j)] = has;
                if (has) ok0[(size_t)c] = 1;
            }
    }
    // ---- the level in HBM; the model takes it only when all of it is there
    DevBuf<double> W1(ctx, (size_t)w_off[n_parents]), C1(ctx, (size_t)c_off[n_parents]);
    DevBuf<int32_t> items1(ctx, (size_t)i_off[n_parents]);
    DevBuf<uint8_t> allowed1(ctx, ok1.size()), allowed0(ctx, ok0.size());
    SyncOnUnwind drain(ctx->stream);
    h2d(ctx, W1.get(), W_ragged, (size_t)w_off[n_parents]);
    h2d(ctx, items1.get(), item_raw, (size_t)i_off[n_parents]);
    h2d(ctx, allowed1.get(), ok1.data(), ok1.size());
    h2d(ctx, allowed0.get(), ok0.data(), ok0.size());
    {
        const int32_t k_max = n_parents ? *std::max_element(sub_clusters, sub_clusters + n_parents) : 0;
        DevBuf<double> part(ctx, (size_t)NMF_GRAM_BLOCKS * k_max * k_max);
        for (int32_t c = 0; c < n_parents; c++)
            if (sub_clusters[c] > 0) nmf_gram(ctx, items_in_cluster[c], sub_clusters[c], W1.get() + w_off[c], part.get(), C1.get() + c_off[c]);
    }
    sync(ctx);
    F->W1 = std::move(W1); F->C1 = std::move(C1); F->items1 = std::move(items1); F->allowed1 = std::move(allowed1);
    if (count) { F->allowed0 = std::move(allowed0); F->has_mask0 = true; }
    F->has_mask1 = count != nullptr;
    F->m_c.assign(items_in_cluster, items_in_cluster + n_parents);
    F->k_c.assign(sub_clusters, sub_clusters + n_parents);
    F->w_off = std::move(w_off); F->c_off = std::move(c_off); F->i_off = std::move(i_off); F->a_off = std::move(a_off);
    F->n_parents = n_parents;
    F->stride = stride;
    publish_blocks(F);
}

fy_foldin_result* foldin_assign(fy_foldin* F, const fy_itemcf_profiles* pf, int32_t iterations, int32_t first_iteration, const double* h0,
                                int32_t rank, int32_t world) {
    Context* ctx = F->ctx;
    const int32_t k = F->prm.number_of_clusters;
    // ---- what the host refuses before any launch
    if (iterations < 0 || first_iteration < 0 || (int64_t)iterations + first_iteration > (int64_t)std::numeric_limits<int32_t>::max())
        FY_FAIL(FY_ERR_INVALID_ARGUMENT, "iterations and first_iteration must be >= 0 and their sum below 2^31");
    if (world < 1 || rank < 0 || rank >= world) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "rank %d of world %d", rank, world);
    if (pf->n_profiles < 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "n_profiles < 0");
    if (pf->base != FY_PROFILE_WHOLE) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "base %d: fy_foldin_assign takes whole profiles only (FY_PROFILE_WHOLE)", pf->base);
    const int64_t n_all = pf->n_profiles;
    if (n_all > 0 && (!pf->user || !pf->start)) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "user or start is NULL");
    if (n_all > 0) {
        if (pf->start[0] != 0) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "start[0] is %lld: the offsets begin at 0", (long long)pf->start[0]);
        for (int64_t p = 0; p < n_all; p++)
            if (pf->start[p + 1] < pf->start[p]) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "start decreases at profile %lld", (long long)p);
        if (pf->start[n_all] > 0 && (!pf->item || !pf->score)) FY_FAIL(FY_ERR_INVALID_ARGUMENT, "item or score is NULL");
        if (pf->start[n_all] > (int64_t)std::numeric_limits<int32_t>::max())
            FY_FAIL(FY_ERR_UNSUPPORTED, "%lld profile entries: at most 2^31 - 1", (long long)pf->start[n_all]);
    }
    if (n_all > (int64_t)std::numeric_limits<int32_t>::max()) FY_FAIL(FY_ERR_UNSUPPORTED, "%lld profiles: at most 2^31 - 1", (long long)n_all);

    // ---- this rank's profiles: a contiguous range of the list given
    const int64_t plo = world > 1 ? n_all * rank / world : 0, phi = world > 1 ? n_all * (rank + 1) / world : n_all;
    const int32_t n = (int32_t)(phi - plo);
    const int64_t e0 = n_all > 0 ? pf->start[plo] : 0;
    const int32_t E = n_all > 0 ? (int32_t)(pf->start[phi] - e0) : 0;
    std::unique_ptr<fy_foldin_result> R(new fy_foldin_result);
    R->ctx = ctx;
    R->k = k;
    fy_foldin_stats& fs = R->stats;
    fs.profiles_asked = n_all;
    fs.profiles_mine = n;
    fs.entries = E;
    R->sub_off.assign((size_t)n + 1, 0);
    if (n == 0) return R.release();
    R->label.assign(pf->user + plo, pf->user + phi);
    R->cluster.assign((size_t)n, -1);
    R->parent.assign((size_t)n, -1);
    R->status.assign((size_t)n, FY_FOLDIN_EMPTY);

    hipStream_t st = ctx->stream;
    EventTimer t_total(ctx), t_ingest(ctx), t_l1(ctx), t_l2(ctx);
    std::vector<int32_t> h_start((size_t)n + 1), h_rowptr((size_t)n + 1, 0), h_arg((size_t)n), h_found((size_t)n), h_block;
    std::vector<int64_t> h_off;
    for (int32_t p = 0; p <= n; p++) h_start[(size_t)p] = (int32_t)(pf->start[plo + p] - e0);
    unsigned long long h_c[FC_N] = {};
    int64_t launches = 0;
    SyncOnUnwind drain(st);      // behind the host ends of the queued copies (and the caller's arrays); the buffers below are released first
    const size_t sp_total = t_total.begin();
    const size_t sp_ingest = t_ingest.begin();

    // ---- ingest: keys, stable sort, last of every run, scan, scatter
    DevBuf<int32_t> start(ctx, (size_t)n + 1), item(ctx, (size_t)E), c_rowptr(ctx, (size_t)n + 1), c_idx(ctx, (size_t)E);
    DevBuf<float> score(ctx, (size_t)E), c_val(ctx, (size_t)E);
    DevBuf<uint8_t> remove;
    DevBuf<unsigned long long> counters(ctx, FC_N);
    counters.zero();
    if (E > 0) {
        h2d(ctx, start.get(), h_start.data(), (size_t)n + 1);
        h2d(ctx, item.get(), pf->item + e0, (size_t)E);
        h2d(ctx, score.get(), pf->score + e0, (size_t)E);
        if (pf->remove) {
            remove.alloc(ctx, (size_t)E);
            h2d(ctx, remove.get(), pf->remove + e0, (size_t)E);
        }
        FoldIn A{};
        A.n = n; A.T = E; A.items = F->prm.number_of_items;
        A.cb = bits_for((int64_t)F->prm.number_of_items - 1);
        A.start = start.get(); A.item = item.get(); A.score = score.get(); A.remove = remove.get();
        DevBuf<uint64_t> keys(ctx, (size_t)E), skeys(ctx, (size_t)E);
        DevBuf<uint32_t> pos(ctx, (size_t)E), spos(ctx, (size_t)E);
        DevBuf<int32_t> keep(ctx, (size_t)E + 1), place(ctx, (size_t)E + 1);
        k_fi_keys<<<grid_for(E), 256, 0, st>>>(A, keys.get(), pos.get(), counters.get());
        FY_KERNEL_CHECK();
        sort_pairs_u64_u32(ctx, keys.get(), skeys.get(), pos.get(), spos.get(), (size_t)E, A.cb + bits_for(n));      // stable
        k_fi_runs<<<grid_for((int64_t)E + 1), 256, 0, st>>>(A, skeys.get(), spos.get(), keep.get(), counters.get());
        FY_KERNEL_CHECK();
        exclusive_scan_i32(ctx, keep.get(), place.get(), (size_t)E + 1);
        k_fi_rowptr<<<grid_for((int64_t)n + 1), 256, 0, st>>>(n, E, A.cb, skeys.get(), place.get(), c_rowptr.get(), counters.get());
        FY_KERNEL_CHECK();
        k_fi_scatter<<<grid_for(E), 256, 0, st>>>(A, skeys.get(), spos.get(), keep.get(), place.get(), c_idx.get(), c_val.get());
        FY_KERNEL_CHECK();
        launches += 6;
    } else {
        FY_HIP(hipMemsetAsync(c_rowptr.get(), 0, ((size_t)n + 1) * sizeof(int32_t), st));
    }
    t_ingest.end(sp_ingest);

    // ---- level 1: every profile on block 0
    const size_t sp_l1 = t_l1.begin();
    DevBuf<double> d_h0;
    if (h0) {
        d_h0.alloc(ctx, (size_t)n * k);
        h2d(ctx, d_h0.get(), h0 + plo * k, (size_t)n * k);
    }
    R->H.alloc(ctx, (size_t)n * k);
    DevBuf<int32_t> arg(ctx, (size_t)n), found(ctx, (size_t)n);
    FoldArgs K{};
    K.n = n; K.rowptr = c_rowptr.get(); K.idx = c_idx.get(); K.val = c_val.get();
    K.blocks = F->blocks.get();
    K.h0 = h0 ? d_h0.get() : nullptr;
    K.iterations = iterations; K.first_iteration = first_iteration; K.ppc = F->prm.ppc ? 1 : 0; K.f = F->prm.normalization_frequency;
    K.out = R->H.get(); K.arg = arg.get(); K.found = found.get();
    k_foldin<<<grid_for((int64_t)n * 64, 256), 256, 0, st>>>(K, k <= 64 ? 1 : 0);
    FY_KERNEL_CHECK();
    launches++;
    t_l1.end(sp_l1);
    d2h(ctx, h_rowptr.data(), c_rowptr.get(), (size_t)n + 1);
    d2h(ctx, h_arg.data(), arg.get(), (size_t)n);
    d2h(ctx, h_c, counters.get(), FC_N);
    sync(ctx);
    fs.entries_out_of_range = (int64_t)h_c[FC_OUT_OF_RANGE];
    fs.entries_superseded = (int64_t)h_c[FC_SUPERSEDED];
    fs.entries_removed = (int64_t)h_c[FC_REMOVED];
    fs.entries_nonpositive = (int64_t)h_c[FC_NONPOSITIVE];
    fs.items_composed = h_rowptr[(size_t)n];
    if (h_rowptr[(size_t)n] < 0 || h_rowptr[(size_t)n] > E) FY_FAIL(FY_ERR_HIP, "fold-in: %d composed items of %d entries", h_rowptr[(size_t)n], E);
    for (int32_t p = 0; p < n; p++) {
        if (h_rowptr[(size_t)p + 1] == h_rowptr[(size_t)p]) continue;      // FY_FOLDIN_EMPTY
        if (h_arg[(size_t)p] < 0 || h_arg[(size_t)p] >= k) { R->status[(size_t)p] = FY_FOLDIN_NO_CLUSTER; continue; }
        R->status[(size_t)p] = FY_FOLDIN_OK;
        R->parent[(size_t)p] = h_arg[(size_t)p];
        R->cluster[(size_t)p] = h_arg[(size_t)p];
    }

    // ---- level 2: every assigned profile on the block of its top-level argmax
    if (F->n_parents) {
        h_block.assign((size_t)n, -1);
        h_off.assign((size_t)n + 1, 0);
        for (int32_t p = 0; p < n; p++) {
            const bool go = R->status[(size_t)p] == FY_FOLDIN_OK;
            if (go) h_block[(size_t)p] = 1 + R->parent[(size_t)p];
            h_off[(size_t)p + 1] = h_off[(size_t)p] + (go ? F->k_c[(size_t)R->parent[(size_t)p]] : 0);
        }
        R->sub_off = h_off;
        const size_t sp_l2 = t_l2.begin();
        DevBuf<int32_t> block_of(ctx, (size_t)n);
        DevBuf<int64_t> out_off(ctx, (size_t)n + 1);
        R->H1.alloc(ctx, (size_t)h_off[(size_t)n]);
        h2d(ctx, block_of.get(), h_block.data(), (size_t)n);
        h2d(ctx, out_off.get(), h_off.data(), (size_t)n + 1);
        K.block_of = block_of.get();
        K.out_off = out_off.get();
        K.h0 = nullptr;      // the sub-runs start uniform
        K.out = R->H1.get();
        k_foldin<<<grid_for((int64_t)n * 64, 256), 256, 0, st>>>(K, 0);
        FY_KERNEL_CHECK();
        launches++;
        t_l2.end(sp_l2);
        d2h(ctx, h_arg.data(), arg.get(), (size_t)n);
        d2h(ctx, h_found.data(), found.get(), (size_t)n);
        sync(ctx);
        for (int32_t p = 0; p < n; p++) {
            if (R->status[(size_t)p] != FY_FOLDIN_OK) continue;
            fs.items_in_parent += h_found[(size_t)p];
            R->cluster[(size_t)p] = -1;
            if (h_found[(size_t)p] == 0) { R->status[(size_t)p] = FY_FOLDIN_EMPTY_IN_PARENT; continue; }
            if (h_arg[(size_t)p] < 0) { R->status[(size_t)p] = FY_FOLDIN_NO_CLUSTER; continue; }
            if (h_arg[(size_t)p] >= F->stride) fs.collisions++;      // the reference's quirk (fy_cluster_refine): kept, nothing is renumbered
            const int64_t id = (int64_t)R->parent[(size_t)p] * F->stride + h_arg[(size_t)p];
            if (id > (int64_t)std::numeric_limits<int32_t>::max()) FY_FAIL(FY_ERR_UNSUPPORTED, "cluster id %lld of profile %d does not fit 32 bits", (long long)id, p);
            R->cluster[(size_t)p] = (int32_t)id;
        }
    }
    t_total.end(sp_total);
    sync(ctx);
    for (int32_t p = 0; p < n; p++) {
        const int32_t s = R->status[(size_t)p];
        if (s != FY_FOLDIN_OK && s != FY_FOLDIN_EMPTY_IN_PARENT) R->parent[(size_t)p] = -1;
        fs.profiles_assigned += s == FY_FOLDIN_OK;
        fs.profiles_empty += s == FY_FOLDIN_EMPTY;
        fs.profiles_no_cluster += s == FY_FOLDIN_NO_CLUSTER;
        fs.profiles_empty_in_parent += s == FY_FOLDIN_EMPTY_IN_PARENT;
    }
    if (E > 0 && fs.profiles_empty != (int64_t)h_c[FC_EMPTY]) FY_FAIL(FY_ERR_HIP, "fold-in: %lld empty profiles by the row pointers, %llu counted", (long long)fs.profiles_empty, h_c[FC_EMPTY]);
    fs.launches = launches;
    fs.ms_ingest = t_ingest.total_ms();
    fs.ms_level1 = t_l1.total_ms();
    fs.ms_level2 = t_l2.total_ms();
    fs.ms_total = t_total.total_ms();
    return R.release();
}

}  // namespace fy
