// fy_rm1.hpp -- the RM1 estimator of a prepared RM2 job (FY_RM2_ESTIMATOR_RM1, include/filmyou.h).
#pragma once
#include <vector>

#include "fy_rm2_request.hpp"

namespace fy {

// Scores the users in `slots` (ascending, inside the rank's share) and fills the list rows of R and the per-phase fields of R->st
// (users_scored, recs, pair_contribs, log_terms, launches, ms_tables / ms_cooc / ms_score / ms_topn) and R->rq (clusters_touched,
// batches).  The side outputs and ms_total of the result are the caller's.  One pass for the full job (every slot of the share)
// and for a request (the slots asked for): a row's bits do not depend on which of the two it came from.
void rm1_score_slots(const RequestView& V, const std::vector<int32_t>& slots, fy_result* R);

// fy_rm2_score_users of an RM1 job
fy_result* rm1_score_users(const RequestView& V, const fy_rm2_request* rq);

}  // namespace fy
