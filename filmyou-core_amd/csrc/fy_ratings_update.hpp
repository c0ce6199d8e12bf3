// fy_ratings_update.hpp -- ratings that take writes: a new COO from a resident one plus a batch of upserts and deletes
// (fy_ratings_apply, include/filmyou.h; the pass and its byte model: DESIGN.md section 4).
#pragma once
#include "fy_common.hpp"

namespace fy {

constexpr int UPD_LDS_KEYS_MAX = 8192;   // largest FY_UPD_LDS_KEYS: 64 KiB of keys beside the 32 KiB user bitmap

// user / item / score / remove_or_null: n entries each, HOST (location FY_HOST) or HBM of the context's GPU (FY_DEVICE).
// Returns a new object (nothing the jobs kept on `R` is carried over, `R` is only read); throws fy::Failure.
// The caller's arrays are no longer read when this returns or throws.
fy_ratings* ratings_apply(Context* ctx, const fy_ratings* R, int64_t n, const int32_t* user, const int32_t* item, const float* score,
                          const uint8_t* remove_or_null, int location, fy_ratings_update_stats* stats_or_null);

}  // namespace fy
