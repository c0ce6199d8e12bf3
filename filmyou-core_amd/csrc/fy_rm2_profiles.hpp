// fy_rm2_profiles.hpp -- RM2 lists for given profiles and pending writes on a prepared job (fy_rm2_score_profiles:
// fy_rm2_profiles.hip).
#pragma once
#include "fy_rm2_request.hpp"

namespace fy {

fy_result* rm2_score_profiles(fy_rm2_job*, const fy_rm2_profiles*);

}  // namespace fy
