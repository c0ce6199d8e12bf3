// fy_rm2_request.hpp -- the restricted RM2 pass (fy_rm2_score_users, fy_rm2_request.hip) and what it sees of a prepared job.
#pragma once
#include <memory>
#include <vector>

#include "fy_prep.hpp"
#include "fy_rm2.hpp"

namespace fy {

// The job handle is opaque outside fy_rm2.hip; this is the part of it a request reads.  Filled by rm2_request_view, which also
// puts the global statistics of a one-rank job in place (what fy_rm2_score does on its first call).
struct RequestView {
    Context* ctx = nullptr;
    fy_rm2_params prm{};
    const Prepared* P = nullptr;
    int32_t slot_lo = 0, slot_hi = 0;        // the slots this rank emits lists for (the full job's share)
    bool have_coll = false;
    const double* stats = nullptr;           // nI global rating sums by dense item + the floor-sum counter (x 100)
    const double* b_rank = nullptr;          // b_i = sum_v x_vi per (cluster, item), rank order
    const long long* walk_rank = nullptr;    // sum of the raters' degrees per (cluster, item), rank order
    const double* usum_slot = nullptr;       // s_v by slot
    // general smoothing (fy_rm2.hpp): P holds r', usum_slot d_v, b_rank b~; the slab's fixed-point scale comes from the row kernel's
    // bounds (fx_rank: per (cluster, item) sum of r' / d_v^2; fx_bounds: per cluster, [3 c + 2] = largest r'), b~ bounds no Gram row
    bool general = false;
    SmoothArgs G{};
    const float* fx_rank = nullptr;          // device, 3 per (cluster, item)
    const float* fx_bounds = nullptr;        // host, 3 per cluster
    std::shared_ptr<void>* state = nullptr;  // what the first request builds and the job keeps (fy_rm2_request.hip: RequestState)
};
void rm2_request_view(fy_rm2_job*, RequestView&);
// the job's parameters and whether collectives are installed, without touching the job (what a request refuses up front)
void rm2_job_peek(const fy_rm2_job*, fy_rm2_params* prm, bool* have_coll);

fy_result* rm2_score_users(fy_rm2_job*, const fy_rm2_request*);

// ---- what the request passes share (fy_rm2_request.hip, fy_rm2_profiles.hip)
// What the first request builds from the ratings and the clustering alone, kept with the cached static part of the job (a later job
// over the same ratings and clustering finds it): host mirrors of the structure the request is planned from and the chunk offsets of
// every user's row for the slab kernel's column chunks.  p(i|C) depends on the job's statistics and is computed per request.
struct RequestState {
    int32_t CH = 0, stride = 0;
    std::vector<int32_t> uid, du2slot, rowptr, csr_idx;
    std::vector<long long> walk;
    DevBuf<int32_t> choff;
};
RequestState& rm2_request_state(const RequestView&);
// p(i|C) of every (cluster, item) in rank order, from the job's statistics (nP doubles, queued on the context's stream)
void rm2_request_p(const RequestView&, double* p_rank);

#ifdef __HIPCC__
struct SlabArgs {
    const int32_t* __restrict__ J;          // [nJ] rows of the slab: item index inside the cluster (rank order)
    int32_t nJ, Ic, CH, nch, pbase, stride;
    int64_t ld;
    const int32_t* __restrict__ rank_pair;
    const int32_t* __restrict__ pair_start;
    const int32_t* __restrict__ csc_slot;
    const float* __restrict__ csc_r;
    const int32_t* __restrict__ choff;
    const int32_t* __restrict__ csr_idx;
    const float* __restrict__ csr_r;
    const double* __restrict__ usum_slot;
    const double* __restrict__ b_rank;
    double* __restrict__ slab;
    const float* __restrict__ fx_rank;      // general smoothing: the row's bound is fx_rank[3 pos] * rmax (null: b_j)
    double rmax;
};
// k_req_slab: the nJ rows J of the cluster's fp64 co-rating matrix, bit-reproducible (fixed-point sums)
void rm2_launch_req_slab(hipStream_t st, const SlabArgs&, const char* who);

// The Jelinek-Mercer term of the request passes, in ONE place: k_req_score and k_prof_score (fy_rm2_profiles.hip) inline the same
// expressions, so a profile that equals its resident row gets that row's bits.
// e_uj = (1 - l)(b_j - x_uj) + l n_others p_j = sum over the neighbours of c_vj, clamped at 0
__device__ __forceinline__ double fy_req_e(double lambda, double b_j, double x_uj, double n_others, double p_j) {
    double e = (1.0 - lambda) * (b_j - x_uj) + lambda * n_others * p_j;
    if (!(e > 0.0)) e = 0.0;
    return e;
}
// ln[w2 g + q_j b_i + a_i e_uj]
__device__ __forceinline__ double fy_req_log_term(double w2, double g, double q_j, double b_i, double a_i, double e_uj) {
    return log(w2 * g + q_j * b_i + a_i * e_uj);
}
// the row's float: the sum of the logs + (n - 1) ln M - n ln U (AbstractRM2Reducer.java:327-329)
__device__ __forceinline__ float fy_req_row_value(double acc, double n, double ln_items, double ln_users) {
    const double pvpi = (n - 1.0) * ln_items - n * ln_users;
    return (float)(acc + pvpi);
}
#endif

}  // namespace fy
