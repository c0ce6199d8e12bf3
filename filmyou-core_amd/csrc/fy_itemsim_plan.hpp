// fy_itemsim_plan.hpp -- what an item-similarity measure is, and which build a job takes: the ONE place where either is decided.
// Host-only and pure: no HIP header, no device call, no global state -- it builds with a plain C++17 compiler and is tested without
// a GPU (tests/test_itemsim_plan_cpu.py).  The full build (fy_itemsim.hip) and the request pass (fy_itemsim_request.hip) ask
// isim_measure / isim_route and run what they say; isim_dispatch is the only switch from a runtime measure to a kernel template.
#pragma once
#include <cstdint>
#include <type_traits>

#include "../../include/filmyou.h"
#include "fy_tuning.hpp"

namespace fy {

enum IsimWeight { ISIM_W_RATING = 0, ISIM_W_ONE = 1, ISIM_W_PEARSON = 2 };      // what a preference weighs in the dot product d
enum IsimNorm { ISIM_A_NONE = 0, ISIM_A_RATERS = 1, ISIM_A_SUMSQ = 2 };        // the norm a_i of the finishing function

// One row of the table of include/filmyou.h ("constant / column transform / norm a_i / similarity") as constants:
//   measure        weight    finishes  counts  a_i        inv_norm  kernel     sweep
//   cosine         rating    -         -       -          yes       COSINE     yes
//   co-occurrence  one       -         -       -          -         COSINE     -
//   Tanimoto       one       yes       yes     raters     -         itself     yes
//   log-likelihood one       yes       yes     raters     -         itself     yes
//   city block     one       yes       yes     raters     -         itself     yes
//   Euclidean      rating    yes       -       sum r^2    -         itself     yes
//   Pearson        centred   -         -       -          -         COSINE     -
struct IsimMeasure {
    int weight;        // IsimWeight
    bool finishes;     // the similarity is a finishing function of (d, a_i, a_j, N); otherwise d is the similarity
    bool counts;       // ... of counts: d and a_i are exact integers whatever the ratings are
    int a;             // IsimNorm
    bool inv_norm;     // the ratings are divided by ||r_.i||: in the weights of the 8-byte walk, in the epilogue of the packed walk
    int kernel;        // the measure the kernel templates are instantiated with: FY_SIMILARITY_COSINE stands for every measure whose
                       // dot product IS the similarity (cosine, co-occurrence, Pearson), a finishing measure for itself
    bool sweep;        // the symmetric build (upper triangle + band sweep) admits it
};
constexpr IsimMeasure isim_measure(int similarity) {
    switch (similarity) {
        case FY_SIMILARITY_COSINE: return {ISIM_W_RATING, false, false, ISIM_A_NONE, true, FY_SIMILARITY_COSINE, true};
        case FY_SIMILARITY_COOCCURRENCE: return {ISIM_W_ONE, false, false, ISIM_A_NONE, false, FY_SIMILARITY_COSINE, false};
        case FY_SIMILARITY_TANIMOTO_COEFFICIENT: return {ISIM_W_ONE, true, true, ISIM_A_RATERS, false, FY_SIMILARITY_TANIMOTO_COEFFICIENT, true};
        case FY_SIMILARITY_LOGLIKELIHOOD: return {ISIM_W_ONE, true, true, ISIM_A_RATERS, false, FY_SIMILARITY_LOGLIKELIHOOD, true};
        case FY_SIMILARITY_CITY_BLOCK: return {ISIM_W_ONE, true, true, ISIM_A_RATERS, false, FY_SIMILARITY_CITY_BLOCK, true};
        case FY_SIMILARITY_EUCLIDEAN_DISTANCE: return {ISIM_W_RATING, true, false, ISIM_A_SUMSQ, false, FY_SIMILARITY_EUCLIDEAN_DISTANCE, true};
        default: return {ISIM_W_PEARSON, false, false, ISIM_A_NONE, false, FY_SIMILARITY_COSINE, false};      // FY_SIMILARITY_PEARSON_CORRELATION
    }
}

// calls f(std::integral_constant<int, M>) with M = the kernel-template measure of `similarity`, and returns what it returns
template <class F>
inline auto isim_dispatch(int similarity, F&& f) {
    switch (isim_measure(similarity).kernel) {
        case FY_SIMILARITY_TANIMOTO_COEFFICIENT: return f(std::integral_constant<int, FY_SIMILARITY_TANIMOTO_COEFFICIENT>{});
        case FY_SIMILARITY_LOGLIKELIHOOD: return f(std::integral_constant<int, FY_SIMILARITY_LOGLIKELIHOOD>{});
        case FY_SIMILARITY_CITY_BLOCK: return f(std::integral_constant<int, FY_SIMILARITY_CITY_BLOCK>{});
        case FY_SIMILARITY_EUCLIDEAN_DISTANCE: return f(std::integral_constant<int, FY_SIMILARITY_EUCLIDEAN_DISTANCE>{});
        default: return f(std::integral_constant<int, FY_SIMILARITY_COSINE>{});
    }
}

constexpr int ISIM_PLAN_FIN_SURV = 512;      // FIN_SURV: entries k_isim_finish sorts per row (fy_itemsim.hip asserts that the two sides agree)

struct IsimRouteInput {
    int similarity;
    int32_t K;                       // maxSimilaritiesPerRow
    int32_t world;
    bool has_threshold;
    double threshold;
    int32_t Ic;                      // items with a kept preference
    bool ratings_fp16_exact, ratings_positive;
    uint64_t total_mem;              // HBM of the device
    int isim_gram, isim_gram_min_items, cooc_pk;      // Tuning
};
struct IsimRoute {
    bool symmetric;      // upper triangle by the RM2 row kernel + band sweep; false: row at a time.  gram_half_build may still decline
                         // (fixed-point scale, chunk count): the caller then runs the row-at-a-time build
    bool packed;         // row at a time: 4-byte CSR entries with the norms in the epilogue; false: the 8-byte-entry walk
};
inline IsimRoute isim_route(const IsimRouteInput& in) {
    const IsimMeasure m = isim_measure(in.similarity);
    IsimRoute r{};
    // packed row kernel when every rating is fp16-exact; Pearson's centred weights are not: it always takes the 8-byte-entry walk
    r.packed = in.ratings_fp16_exact && in.cooc_pk && m.weight != ISIM_W_PEARSON;
    r.symmetric = [&] {
        if (!m.sweep) return false;      // co-occurrence, Pearson: row at a time
        // the count measures multiply ones: the fixed-point sums are exact integers whatever the ratings are
        if (in.isim_gram == 0 || in.world != 1 || !in.cooc_pk || (!m.counts && (!in.ratings_fp16_exact || !in.ratings_positive)) ||
            in.K > ISIM_PLAN_FIN_SURV / 2 || (in.has_threshold && !(in.threshold > 0.0)))
            return false;
        // cosine takes this build from isim_gram_min_items items on.  The other measures take it only when it is forced
        // (FY_ISIM_GRAM=1): their sweep has not been shown faster than their row-at-a-time build.
        if (in.isim_gram < 0 && (in.similarity != FY_SIMILARITY_COSINE || in.Ic < in.isim_gram_min_items)) return false;
        if ((uint64_t)in.Ic * (uint64_t)round_up(in.Ic, 256) * 4 > in.total_mem / 3) return false;      // the fp32 matrix must fit comfortably
        return true;
    }();
    return r;
}

}  // namespace fy
