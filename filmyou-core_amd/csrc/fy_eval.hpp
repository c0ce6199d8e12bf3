// fy_eval.hpp -- offline evaluation: hold-out split of resident ratings, a list result from rows, and the ranking metrics of a list
// result where it lies in HBM (fy_ratings_holdout, fy_result_create_lists, fy_eval_*; include/filmyou.h).
#pragma once
#include "fy_common.hpp"

// What fy_eval_prepare leaves in HBM: the relevant test entries as one ascending row of items per user, found by two binary searches.
struct fy_eval {
    fy::Context* ctx = nullptr;
    fy_eval_params p{};
    int32_t n_users = 0;                 // distinct users with a relevant entry
    int32_t n_entries = 0;               // relevant entries
    fy::DevBuf<uint32_t> user;           // n_users ids, ascending as unsigned 32-bit patterns
    fy::DevBuf<int32_t> start;           // n_users + 1 row starts into item / gain
    fy::DevBuf<uint32_t> item;           // n_entries, ascending inside a row
    fy::DevBuf<double> gain;             // n_entries (graded gains only)
    fy::DevBuf<double> idcg;             // n_users x n_cutoffs
    fy::DevBuf<double> discount;         // 1 / log2(p + 1), p = 1 .. cutoffs[n - 1]
};

namespace fy {

// Throw fy::Failure; the outputs are untouched on failure.
void ratings_holdout(Context* ctx, const fy_ratings* R, double fraction, uint64_t seed, fy_ratings** train, fy_ratings** test);
fy_result* result_create_lists(Context* ctx, int64_t n, const int32_t* user, const int32_t* item, const float* value, int location);
fy_eval* eval_prepare(Context* ctx, const fy_eval_params* p, const fy_ratings* test);
void eval_lists(fy_eval* E, fy_result* lists, fy_eval_sums* out, int32_t* per_user_id, double* per_user);
// the error sums of an estimates result (kind 4) against the truth entries at the same positions; p may be NULL (no clamp)
void eval_estimates(Context* ctx, fy_result* estimates, const fy_ratings* truth, const fy_eval_error_params* p, fy_eval_errors* out);

}  // namespace fy
