// fy_itemcf_profiles.hpp -- item-based lists for given profiles on a prepared similarity job (fy_itemcf_recommend_profiles:
// fy_itemcf_profiles.hip).
#pragma once
#include "fy_itemcf_request.hpp"

namespace fy {

// items_only: NULL, or a filter with has_users == 0 (itemsFile alone)
fy_result* itemcf_recommend_profiles(fy_itemsim_job*, const fy_itemcf_params*, const fy_itemcf_profiles*, const fy_itemcf_filter* items_only);

}  // namespace fy
