// fy_rm2_request.hpp -- the restricted RM2 pass (fy_rm2_score_users, fy_rm2_request.hip) and what it sees of a prepared job.
#pragma once
#include <memory>

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

fy_result* rm2_score_users(fy_rm2_job*, const fy_rm2_request*);

}  // namespace fy
