// fy_rm2.hpp -- internal interface between the C ABI (fy_api.hip) and the job implementations.
#pragma once
#include <memory>

#include "fy_common.hpp"

// result rows live in HBM until an accessor asks for them
struct fy_result {
    fy::Context* ctx = nullptr;
    int kind = 0;   // 0 = RM2, 1 = item-sim, 2 = item-CF lists, 3 = item pairs, 4 = item-CF estimates (one row per asked pair), 5 = item-CF explanations
    int64_t n = 0;
    fy::DevBuf<int32_t> d_key0, d_key1, d_aux;
    fy::DevBuf<float> d_value;
    fy::DevBuf<int32_t> d_user_id, d_item_id;
    fy::DevBuf<double> d_user_sum, d_icoll;
    double total_sum = 0.0;
    fy_stats st{};
    bool has_request_stats = false;   // a result of fy_rm2_score_users
    fy_rm2_request_stats rq{};
    bool has_rm2_profile_stats = false;       // a result of fy_rm2_score_profiles
    fy_rm2_profile_stats rpf{};
    bool has_itemsim_request_stats = false;   // a result of fy_itemsim_rows
    fy_itemsim_request_stats irq{};
    bool has_itemcf_request_stats = false;    // a result of fy_itemcf_recommend_prepared
    fy_itemcf_request_stats crq{};
    bool has_itemcf_profile_stats = false;    // a result of fy_itemcf_recommend_profiles
    fy_itemcf_profile_stats cpf{};
    bool has_itemcf_estimate_stats = false;   // a result of fy_itemcf_estimate_prepared / fy_itemcf_estimate_ratings (kind 4)
    fy_itemcf_estimate_stats est{};
    // a result of fy_itemcf_because_prepared (kind 5): rows = the listed contributors; per asked pair (bp_n of them) the ids, the
    // estimate, its status, the count of contributors and the first row (bp_n + 1); per row the preference
    bool has_itemcf_because_stats = false;
    fy_itemcf_because_stats bec{};
    int64_t bp_n = 0;
    fy::DevBuf<int32_t> d_bp_user, d_bp_item, d_bp_status, d_bp_cnt, d_bp_start;
    fy::DevBuf<float> d_bp_est, d_pref;
    bool because_on_host = false;
    std::vector<int32_t> h_bp_user, h_bp_item, h_bp_status, h_bp_cnt;
    std::vector<int64_t> h_bp_start;
    std::vector<float> h_bp_est, h_pref;
    // host mirrors, filled on first access
    bool rows_on_host = false, sums_on_host = false;
    std::vector<int32_t> h_key0, h_key1, h_aux, h_user_id, h_item_id;
    std::vector<float> h_value;
    std::vector<double> h_user_sum, h_icoll;
};

namespace fy {
// The smoothing of a job (include/filmyou.h, FY_RM2_SMOOTHING_*): c_vi = w x_vi + beta_v p_i with x_vi = r'_vi / d_v.
// Jelinek-Mercer keeps the code it always had; the two other methods ("general") run the second instantiations of the statistics
// pass and the table kernels, and the scalar w^2 = 1 wherever Jelinek-Mercer has (1 - lambda)^2.
struct Smoothing {
    int method = 0;        // 0 Jelinek-Mercer, 1 Dirichlet prior, 2 absolute discounting
    double param = 0.0;    // lambda | mu | delta
    bool general() const { return method != 0; }
    // the scale of the Gram part of a term: (1 - lambda)^2, or w^2 = 1 (the expression Jelinek-Mercer always had, unchanged)
    double w2_of(double lambda) const { return method == 0 ? (1.0 - lambda) * (1.0 - lambda) : 1.0; }
};
inline Smoothing smoothing_of(const fy_rm2_params& p) {
    Smoothing s;
    s.method = (p.flags & FY_RM2_SMOOTHING_DIRICHLET) ? 1 : (p.flags & FY_RM2_SMOOTHING_ABSOLUTE_DISCOUNT) ? 2 : 0;
    s.param = p.lambda;
    return s;
}
#ifdef __HIPCC__
// What the kernels of a general-smoothing job read besides the arrays every job has: beta_v and n_v by slot (d_v is in the place
// of s_v), S2 = sum of beta_v^2 per cluster, and how the statistics pass formed b~ (PairPass::bt_scale / bt_by_n, fy_rm2.hip).
struct SmoothArgs {
    const double* __restrict__ beta_slot;
    const int32_t* __restrict__ deg_slot;
    const double* __restrict__ s2_cluster;
    double bt_scale;
    int32_t bt_by_n;
};
// e~_uj = (b~_j - beta_u x_uj) + p_j (S2 - beta_u^2) = sum_{v != u} beta_v c_vj, both differences clamped at 0.  beta_u x_uj is
// formed by the statistics pass's own rounded products, so a column whose only rater is u cancels to exactly 0 (-> ln 0 = -inf,
// as Jelinek-Mercer's (1 - l)(b_j - x_uj) does).
__device__ __forceinline__ double fy_e_general(double bt_j, double p_j, double r_uj, double d_u, double n_u, double beta_u, double s2,
                                               double bt_scale, int32_t bt_by_n) {
    const double inv = 1.0 / d_u;
    const double wt = __dmul_rn(__dmul_rn(r_uj, inv), inv);
    const double bx = __dmul_rn(bt_scale, bt_by_n ? __dmul_rn(wt, n_u) : wt);
    double e1 = bt_j - bx, e2 = s2 - __dmul_rn(beta_u, beta_u);
    if (!(e1 > 0.0)) e1 = 0.0;
    if (!(e2 > 0.0)) e2 = 0.0;
    return e1 + p_j * e2;
}
#endif
fy_rm2_job* rm2_prepare(Context*, const fy_rm2_params*, const fy_ratings*, int64_t n_map, const int32_t* map_user,
                        const int32_t* map_cluster, const int32_t* cluster_count);
void rm2_partial_stats(fy_rm2_job*, double** buf, int64_t* len);
void rm2_stats_layout(fy_rm2_job*, int64_t* n_item_slots, int64_t* n_user_slots);
void rm2_set_global_stats(fy_rm2_job*, const double* gathered, int32_t world);
void rm2_set_collectives(fy_rm2_job*, const fy_collectives*);
fy_result* rm2_score(fy_rm2_job*);
void rm2_job_destroy(fy_rm2_job*);
fy_result* itemsim_build(Context*, const fy_itemsim_params*, const fy_ratings*);
struct Prepared;
// upper triangle of the weighted co-rating Gram of a one-cluster structure as fp32 (fy_rm2.hip; used by fy_itemsim.hip)
bool gram_half_build(Context* ctx, const Prepared& P, const float* csc_w, const float* bounds3, float* G, int64_t ldm, double* ms_tables,
                     double* ms_walk, const float* csr_ones = nullptr /* column side all ones (in CSR order) instead of the ratings: co-rating counts */);
void cluster_assign(Context*, int32_t n_rows, int32_t k, const double* H, int location, int32_t first_user, int32_t cluster_offset,
                    int32_t n_clusters, int32_t* user_out, int32_t* cluster_out, int32_t* count_inout);
void nmf_factorize(Context*, const fy_nmf_params*, const fy_ratings*, double* H, double* W, fy_stats* st);
fy_result* itemcf_recommend(Context*, const fy_itemcf_params*, const fy_ratings*, fy_result* similarities);
fy_result* itemcf_recommend_filtered(Context*, const fy_itemcf_params*, const fy_itemcf_filter*, const fy_ratings*, fy_result* similarities);
fy_ratings* ratings_shifted(Context*, const fy_ratings*, float shift);
fy_result* itemsim_pairs(Context*, fy_result* similarities);

constexpr int TOPN_LIST_MAX = 2048;   // longest list of the top-N kernels (TOPN_MAX of fy_rm2_kernels.hpp)
// top-N over rows of a dense score matrix (NaN = not a candidate): launch_topn (fy_rm2_launch.hpp): k_topn_fast or k_topn_long, then k_topn_select.
// n_out[u] rows are written at out_off[u] for u in [0, n_rows); item ids come from rank_item_raw[column].
void launch_topn_rows(Context* ctx, hipStream_t st, const float* S, int64_t ldS, int32_t n_cols, int32_t n_rows,
                      const int32_t* n_out, const int32_t* out_off, const int32_t* rank_item_raw, const int32_t* slot2du,
                      const int32_t* uid, int32_t slot0, int32_t aux_value, int32_t* out_user, int32_t* out_item,
                      float* out_score, int32_t* out_aux, int32_t* overflow, int32_t* any_overflow, int32_t top_n_hint = 0);
}  // namespace fy
