// fy_rm2_plan.hpp -- how an RM2 job scores its clusters, decided on the host from plain numbers (fy::plan_job).
// Host-only and pure: no HIP header, no device call, no global state -- it builds with a plain C++17 compiler and is tested without
// a GPU (tests/test_rm2_plan_cpu.py).  fy::rm2_score (fy_rm2.hip) fills a PlanInput, calls plan_job and runs what the JobPlan says.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/filmyou.h"
#include "fy_tuning.hpp"

namespace fy {

// limits of the kernels the plan is made for (fy_rm2_kernels.hpp; fy_rm2.hip asserts that the two sides agree)
constexpr int PLAN_TOPN_MAX = 2048;          // TOPN_MAX: longest list
constexpr int PLAN_TOPN_SAMPLE = 1024;       // TOPN_SAMPLE: seed columns the one-wave seed sort holds
constexpr int PLAN_TOPN_LONG = 256;          // TOPN_LONG: lists longer than this take k_topn_long
constexpr int PLAN_SEED_CHUNKS_MAX = 40;     // SEED_CHUNKS_MAX: widest seed of the branch and bound
constexpr int PLAN_PRUNE_BLOCK = 256;        // PRUNE_BLOCK: candidate block of the branch and bound
constexpr int PLAN_STRAY_UCAP = 32768;       // STRAY_UCAP: users of a panel-mode cluster

// what the planning refuses: fy::rm2_score turns it into FY_FAIL(code, msg)
struct PlanError {
    int code;
    std::string msg;
};
#define FY_PLAN_FAIL(code_, ...)                          \
    do {                                                  \
        char _m[512];                                     \
        snprintf(_m, sizeof(_m), __VA_ARGS__);            \
        throw fy::PlanError{code_, std::string(_m)};      \
    } while (0)

// picks the chunk width for a cluster with Ic items: whole row when it fits the LDS budget.  Chunks are multiples of 256
// columns whenever there are several (a wave of the epilogue then owns exactly one 256-column block, fy_rm2.hip).
inline void pick_chunks(int32_t Ic, int32_t max_ch, int32_t& CH, int32_t& nch) {
    if (Ic <= max_ch) {
        CH = (int32_t)round_up(Ic > 0 ? Ic : 1, 64);
        nch = 1;
    } else {
        const int32_t cap = max_ch >= 256 ? (max_ch / 256) * 256 : max_ch;
        const int32_t gran = max_ch >= 256 ? 256 : 64;
        nch = (int32_t)ceil_div(Ic, cap);
        CH = (int32_t)std::min<int64_t>(cap, round_up(ceil_div(Ic, nch), gran));
        nch = (int32_t)ceil_div(Ic, CH);
    }
}

// Exponent k of the fixed-point scale 2^k of a cluster (CoocArgs::fx_scale): the largest k with (largest contribution) * 2^k < 2^51
// and (largest possible Gram entry) * 2^k < 2^62, from the cluster's bounds (sum and maximum of the segment weights r / s^2 per
// item, largest rating).  Returns a negative number when the bounds are unusable (the fp64 path is taken then).
inline int fx_exponent(const float* bounds3) {
    const double wsum = bounds3[0], wmax = bounds3[1], rmax = bounds3[2];
    if (!(wsum > 0.0) || !(wmax > 0.0) || !(rmax > 0.0) || !std::isfinite(wsum * rmax)) return -1;
    const int k1 = 51 - (std::ilogb(wmax * rmax) + 1), k2 = 62 - (std::ilogb(wsum * rmax) + 1);
    const int k = std::min(std::min(k1, k2), 1000);
    return k >= 24 ? k : -1;
}

// user slices (workgroups per column chunk) of a scoring launch over `nb` users and `chunks` column chunks: a wave walks up to
// users_per_wave users, but a small batch (one cluster of many: 3 250 users at 50 clusters) is cut finer so that the launch
// still has ~8 workgroups per CU -- with 16 users per wave such a launch had 102 workgroups for 256 CUs (1.4 ms per cluster
// for work that takes 0.14 ms of the one-cluster job)
inline int score_slices(int num_cus, const Tuning& tune, int64_t nb, int chunks) {
    const int64_t coarse = ceil_div(nb, 4 * (int64_t)tune.users_per_wave), finest = ceil_div(nb, 4);
    const int64_t fill = ceil_div(8 * (int64_t)num_cus, std::max(1, chunks));
    return (int)std::max<int64_t>(1, std::min<int64_t>(tune.max_slices, std::min(finest, std::max(coarse, fill))));
}

// Super-blocks of the bound pass (k_score_sup): the fine 256-column blocks [seed_blocks, nblk) in at most 64 groups -- the first 48
// one block each (that is where survivors are: the columns are in popularity order and RM2 scores fall steeply with it), the rest
// in 16 groups of growing width.  first[s] .. first[s + 1] are the fine blocks of group s.
inline void sup_block_map(int seed_blocks, int nblk, std::vector<int32_t>& first) {
    first.clear();
    const int R = std::max(0, nblk - seed_blocks);
    if (R <= 64) {
        for (int s = 0; s <= R; s++) first.push_back(seed_blocks + s);
        return;
    }
    for (int s = 0; s < 48; s++) first.push_back(seed_blocks + s);
    const int rem = R - 48;
    int64_t cum = 0;
    for (int k = 0; k < 16; k++) {            // widths ~ (k + 1): 1 + 2 + .. + 16 = 136 parts
        first.push_back(seed_blocks + 48 + (int32_t)((int64_t)rem * cum / 136));
        cum += k + 1;
    }
    first.push_back(nblk);
    for (size_t k = 1; k < first.size(); k++) first[k] = std::max(first[k], first[k - 1]);      // (monotone; a group may be empty)
}

// one cluster's launch plan
struct Plan {
    int c;
    int32_t Uc, sbase, pbase, Ic, a, b, CH, nch, q0, nq;
    int64_t ldm, B;
    bool pack24, prune, coop, half, panel;
    bool psym;       // symmetric panel mode: head rows x head columns by a half walk + mirror, head rows x tail columns not at all (k_panel_colmax)
    bool flat;       // one of many small unpruned clusters whose kernels run in ONE launch each (fy_rm2_kernels.hpp: FlatDesc)
    int32_t panel_cols, nsub;
    int64_t ldb64;
    // panel mode: the rows from p_eff on ("tail rows") are walked only over their first tail_chunks chunks (= the columns in
    // front of p_eff, a chunk boundary behind the panel); their block bounds behind p_eff come from k_tail_blocks' CSR
    int32_t tail_chunks, p_eff, tail_width;
    int32_t nblk;
    int64_t ldb;
    // symmetric walk from the unpopular side (CoocArgs::half == 2): a row stores its own chunk from its diagonal block on and the WHOLE
    // chunks in front of it, nothing behind its own chunk -- the off-diagonal chunk rectangles are walked by the rows with few raters,
    // whose raters' slices in the popular chunks are long (full segments).  Chunks of whole 256-column blocks only.
    bool rect;
};

// everything the planning reads: plain numbers and host vectors
struct PlanInput {
    // of the prepared structure (fy_prep.hpp: Prepared)
    int32_t K = 0, nU = 0;
    std::vector<int32_t> csize, ucstart, pcstart, cluster_q;   // K, K+1, K+1, K+1
    std::vector<int64_t> cluster_deg2;
    int64_t sum_deg2 = 0;
    bool ratings_fp16_exact = false;
    std::vector<float> fx_bounds;        // 3 per cluster, or empty
    // of fy_rm2_params
    int32_t number_of_recommendations = 0, rank = 0, world = 1;
    double lambda = 0.0;
    bool general_smoothing = false;      // Dirichlet prior / absolute discounting: w^2 = 1 and fx_bounds are taken over r' and d_v
    int64_t workspace_bytes = 0;
    Tuning tune;
    uint64_t total_mem = 0;              // HBM of the device
    bool sharded = false, have_coll = false;
    // the slots every rank emits lists for (owner_range, fy_rm2.hip): taken AFTER plan_count_balanced, which they depend on
    std::vector<int32_t> own_lo, own_hi;
    int64_t n_recs = 0;                  // list entries this rank emits (from the device); 0: no cluster is planned
};

// the seed of the branch and bound, resolved from the list length
struct SeedPlan {
    int seed_chunks;
    bool long_seed, short_seed_ok;
};
inline SeedPlan plan_seed(const Tuning& tune, int32_t number_of_recommendations) {
    SeedPlan s{tune.seed_chunks, false, false};
    // tau_u is the N-th best of the seed scores: a seed of only a few N columns gives a weak threshold and many survivors
    // (Netflix shape, N = 100: 2.7 % of the blocks survive a 256-column seed, 0.1 % a 512-column one)
    // (round 4: also for long lists -- the reference's default is N = 1000, RMRecommenderDriver.java:95 -- whose seed is 5 N columns too:
    // 5120 of ML-25M's 59 047; up to round 3 the seed stopped at 1024 columns, whose 1000th best is no threshold at all, and such
    // jobs took the plain full pass)
    if (s.seed_chunks == 0) s.seed_chunks = (int)std::min<int64_t>(PLAN_SEED_CHUNKS_MAX, std::max<int64_t>(1, ceil_div(5 * (int64_t)number_of_recommendations, 256)));
    // lists the one-wave seed sort cannot hold (k_topn_seed: at most TOPN_SAMPLE seed columns, lists of at most TOPN_LONG items) take
    // k_topn_long in its seed / merge modes
    s.long_seed = s.seed_chunks * 256 > PLAN_TOPN_SAMPLE || number_of_recommendations > PLAN_TOPN_LONG;
    s.short_seed_ok = tune.seed_forced || 5 * (int64_t)number_of_recommendations <= 4 * 256;     // (the cooperative path's limit)
    return s;
}

// packed (24-bit) matrix rows only where bandwidth matters: small clusters keep exact fp32 rows (their scores are small, and the
// reference's own fixture is asserted with an ABSOLUTE 1e-4, T/util/HadoopIntegrationTest.java:53).  A packed cluster's matrix is
// scaled by 2^-c so that every entry is < 1 (FY_P24_SHIFT): G[j][i] = w2 sum_v (r_vj / s_v^2) r_vi <= w2 * (largest column sum
// of r / s^2) * (largest rating), the bounds of the fixed-point scale.
struct PackPlan {
    std::vector<float> h_gscale;         // [cluster]: 2^-c
    std::vector<int32_t> h_cshift;       // [cluster]: c
    std::vector<char> pack24;            // [cluster]
};
inline PackPlan plan_pack24(const PlanInput& in) {
    const Tuning& tune = in.tune;
    const int K = in.K;
    const double lambda = in.lambda;
    const bool pack24_allowed = tune.pack24 != 0;
    PackPlan out;
    std::vector<float>& h_gscale = out.h_gscale;
    std::vector<int32_t>& h_cshift = out.h_cshift;
    std::vector<char>& cluster_pack24 = out.pack24;
    h_gscale.assign((size_t)K, 1.0f);
    h_cshift.assign((size_t)K, 0);
    cluster_pack24.assign((size_t)K, 0);
    for (int c = 0; c < K; c++) {
        const int32_t Ic_c = in.pcstart[c + 1] - in.pcstart[c];
        if (!pack24_allowed || Ic_c < tune.pack24_min_items || in.fx_bounds.size() < 3 * (size_t)(c + 1)) continue;
        const double w2 = in.general_smoothing ? 1.0 : (1.0 - lambda) * (1.0 - lambda);
        const double gmax = w2 * (double)in.fx_bounds[3 * (size_t)c] * (double)in.fx_bounds[3 * (size_t)c + 2];
        if (!(gmax >= 0.0) || !std::isfinite(gmax)) continue;                     // unusable bound: fp32 rows
        const int cs = gmax > 0.0 ? std::max(0, std::ilogb(gmax) + 1) : 0;
        if (cs > 64) continue;
        cluster_pack24[c] = 1;
        h_cshift[c] = cs;
        h_gscale[c] = std::ldexp(1.0f, -cs);
    }
    return out;
}

// Scoring ownership of the users by equal COUNTS instead of equal work (owner_range, fy_rm2.hip): a job whose one neighbourhood is
// scored cooperatively by all ranks.
inline bool plan_count_balanced(const PlanInput& in) {
    const Tuning& tune = in.tune;
    const SeedPlan seed = plan_seed(tune, in.number_of_recommendations);
    const bool pack24_allowed = tune.pack24 != 0;
    bool count_balanced = false;
    if (in.world > 1 && !in.sharded && in.have_coll && tune.coop && tune.prune && pack24_allowed) {     // (a cooperative cluster must be a packed one: checked per plan)
        int nonempty = 0, c1 = -1;
        for (int c = 0; c < in.K; c++)
            if (in.csize[c] > 0) { nonempty++; c1 = c; }
        if (nonempty == 1) {   // one neighbourhood: it is scored cooperatively when it is big enough for the branch and bound
            const int32_t Ic1 = in.pcstart[c1 + 1] - in.pcstart[c1];
            count_balanced = Ic1 >= tune.pack24_min_items && Ic1 >= tune.prune_min_items && ceil_div(Ic1, PLAN_PRUNE_BLOCK) < 0xFFFF &&
                             in.nU >= in.world && seed.short_seed_ok && !seed.long_seed;
        }
    }
    return count_balanced;
}

// bytes a cluster holds in a flat batch: its matrix, its score rows, its item list
inline int64_t flat_need(const Plan& p) {
    return (int64_t)p.Ic * p.ldm * (p.pack24 ? 3 : 4) + (int64_t)(p.b - p.a) * p.ldm * 4 + (int64_t)p.Ic * p.nch * 12 + 4096;
}

struct JobPlan {
    std::vector<Plan> plans;             // the clusters that hold users of this rank
    std::vector<float> h_gscale;
    std::vector<int32_t> h_cshift;
    bool use_pk = false;                 // packed CSR for the row kernel
    bool long_seed = false, short_seed_ok = false;
    int seed_chunks = 0;                 // resolved (Tuning::seed_chunks == 0: from the list length)
    bool count_balanced = false;
    int64_t max_Ic = 0;
    int32_t eff_top = 0;
    int64_t ws = 0;                      // score scratch per batch of users
    int64_t flat_budget = 0;
    bool any_panel = false, two_phase = false;
    std::vector<int> group_of;           // [plan]: panel group (clusters outside panel mode are in group 0)
    int n_groups = 1;
    int NS = 0;                          // lanes
    bool any_coop = false, any_tail = false, any_half = false;
    size_t co_all = 1;                   // chunk offsets of the largest cluster (no reader in the library any more: the tables' layout is layout_tables'; pinned by the golden plans)
    // elements of the per-lane buffers
    size_t m_el = 1, s_el = 1, ov_el = 1, bm_el = 1, ub_el = 1, am_el = 1, gp_el = 1, b64_el = 1, a64_el = 1, is_el = 1;
};

inline JobPlan plan_job(const PlanInput& in) {
    const Tuning& tune0 = in.tune;
    JobPlan jp;
    const SeedPlan seed = plan_seed(tune0, in.number_of_recommendations);
    Tuning tune = tune0;
    tune.seed_chunks = seed.seed_chunks;
    const bool long_seed = seed.long_seed, short_seed_ok = seed.short_seed_ok;
    jp.seed_chunks = seed.seed_chunks;
    jp.long_seed = long_seed;
    jp.short_seed_ok = short_seed_ok;
    const bool use_pk = tune.cooc_pk && in.ratings_fp16_exact;   // packed CSR for the row kernel
    jp.use_pk = use_pk;
    PackPlan pack = plan_pack24(in);
    const std::vector<char>& cluster_pack24 = pack.pack24;
    jp.h_gscale = std::move(pack.h_gscale);
    jp.h_cshift = std::move(pack.h_cshift);
    jp.count_balanced = plan_count_balanced(in);
    const int K = in.K;
    const int32_t lo = in.own_lo[(size_t)in.rank], hi = in.own_hi[(size_t)in.rank];

    // ---- clusters that hold users of this rank
    int64_t max_Ic = 0;
    for (int c = 0; c < K; c++) {
        if (in.csize[c] == 0) continue;
        const int32_t a = std::max(lo, in.ucstart[c]), b = std::min(hi, in.ucstart[c + 1]);
        if (a < b) max_Ic = std::max<int64_t>(max_Ic, in.pcstart[c + 1] - in.pcstart[c]);
    }
    const int32_t eff_top = (int32_t)std::min<int64_t>(in.number_of_recommendations, max_Ic);
    if (eff_top > PLAN_TOPN_MAX)
        FY_PLAN_FAIL(FY_ERR_UNSUPPORTED, "min(numberOfRecommendations, items per cluster) = %d exceeds the top-N kernel limit %d", eff_top, PLAN_TOPN_MAX);
    jp.max_Ic = max_Ic;
    jp.eff_top = eff_top;
    if (!(in.n_recs > 0 && max_Ic > 0)) return jp;

    const int64_t ws = in.workspace_bytes > 0 ? in.workspace_bytes : tune.workspace_default;
    jp.ws = ws;
    const int max_ch_lds = tune.cooc_max_ch;   // fp64 accumulators in LDS

    // ---- per-cluster plan; the clusters are spread over up to four "lanes" (HIP streams with their own M / score
    // scratch): the tail of one cluster's launches -- its heaviest user sits on a single wave for milliseconds, and
    // most of its M rows have a handful of raters -- overlaps the next clusters' work instead of idling the chip.
    std::vector<Plan>& plans = jp.plans;
    for (int c = 0; c < K; c++) {
        Plan p{};
        p.c = c;
        p.Uc = in.csize[c];
        if (p.Uc == 0) continue;
        p.sbase = in.ucstart[c];
        p.pbase = in.pcstart[c];
        p.Ic = in.pcstart[c + 1] - p.pbase;
        p.a = std::max(lo, p.sbase);
        p.b = std::min(hi, p.sbase + p.Uc);
        if (p.a >= p.b || p.Ic == 0) continue;
        p.ldm = round_up(p.Ic, 256);
        p.pack24 = cluster_pack24[c] != 0;
        // (the item ids of the row kernel hold the chunk in 8 bits, k_item_list: at most 255 chunks per row -- a forced
        // FY_COOC_MAX_CH too small for that is widened)
        pick_chunks(p.Ic, std::max<int>(max_ch_lds, (int)round_up(ceil_div(p.Ic, 255), 256)), p.CH, p.nch);
        if (p.nch >= 256) FY_PLAN_FAIL(FY_ERR_UNSUPPORTED, "cluster %d: %d items need %d column chunks (limit 255)", c, p.Ic, p.nch);
        p.q0 = in.cluster_q[c];
        p.nq = in.cluster_q[c + 1] - p.q0;
        // branch-and-bound over 256-column blocks: only where the matrix is big enough for the bound pass to pay
        p.nblk = (int32_t)ceil_div(p.Ic, PLAN_PRUNE_BLOCK);
        p.ldb = round_up(p.nblk, 256);
        // (the threshold is the N-th best of at most 1024 seed scores: for lists longer than ~200 items it is too weak --
        // N = 1000 at ML-25M shape: 77 % of the blocks survive and the three passes cost twice the plain one)
        // (and clusters of a few hundred users are not pruned at all: their seed thresholds are weak -- at 400 clusters of ML-25M
        // shape, 406 users each, 16-44 % of the blocks survive and the plain full pass is 1.6x faster than any pruned variant)
        // (long lists: the seed is 5 N columns; where that is more than a third of the cluster's items the bound has nothing left to
        // exclude and the plain full pass is taken)
        p.prune = tune.prune && p.pack24 && p.Ic >= tune.prune_min_items && p.nblk < 0xFFFF && p.Uc >= tune.prune_min_users &&
                  (tune.seed_forced || 3 * (int64_t)tune.seed_chunks * 256 <= (int64_t)p.Ic);
        if (jp.count_balanced && !p.prune) FY_PLAN_FAIL(FY_ERR_STATE, "internal: count-balanced ownership without a cooperative cluster");
        // all ranks hold users of this cluster and can talk to each other: score it together, every rank with its
        // share of the matrix rows (score_cluster_coop)
        p.coop = false;
        if (p.prune && tune.coop && short_seed_ok && !long_seed && ((in.world > 1 && in.have_coll) || tune.coop_force)) {
            p.coop = true;
            for (int k = 0; k < in.world; k++) {
                const int32_t lo_k = in.own_lo[(size_t)k], hi_k = in.own_hi[(size_t)k];
                if (std::max(lo_k, p.sbase) >= std::min(hi_k, p.sbase + p.Uc)) p.coop = false;
            }
        }
        // symmetric walk: packed rows only (small clusters keep exact fp32 rows and the plain walk); a cooperative rank
        // owns whole rows of the matrix, so it walks them whole
        p.half = tune.cooc_half && p.pack24 && !p.coop && p.nch < 256;
        p.panel = false;
        p.panel_cols = 0;
        p.tail_chunks = 0;
        p.p_eff = p.Ic;
        p.tail_width = 0;
        p.nsub = (int32_t)ceil_div(p.Ic, 64);
        p.ldb64 = round_up(p.nsub, 256);
        plans.push_back(p);
    }
    {   // column-panel mode: many pruned clusters on this rank (the reference's regime: numberOfClusters ~ 50)
        int n_pruned = 0;
        for (auto& p : plans) n_pruned += (p.prune && !p.coop) ? 1 : 0;
        // Long lists are pruned only where a few big clusters keep their dense matrices.  Measured at 50 clusters of ML-25M shape with
        // N = 1000 (round 4): 41 % of the (user, block) pairs survive the bound of a 3 250-user cluster and 10 M of them lie behind
        // the panel -- 14.9 s per job against 0.67 s for the plain full pass; one cluster: 14 % survive, 271 against 471 ms.
        // (and on dense per-cluster matrices instead of panels: 29 568 184 of 29 568 241 blocks survive -- a 3 250-user neighbourhood's
        // 1000th best score is no threshold -- every cluster falls back to the full pass, 957 ms)
        if (long_seed && n_pruned >= tune.panel_min_clusters && !tune.seed_forced) {
            for (auto& p : plans)
                if (!p.coop) p.prune = false;
            n_pruned = 0;
        }
        // A cluster that takes the plain full pass reads its WHOLE matrix.  The symmetric walk + mirror pass pays where the walk is
        // bound by its pair visits (one cluster of ML-25M shape: 6.5e9 visits, 8 ms; the mirror 2.6 ms); a cluster of many (50
        // clusters: 1.3e8 visits each for 2.6e9 matrix elements) is bound by the rows it WRITES -- 1.65 ms for the half matrix plus 4.3 ms
        // to mirror 7.8 GB, against ~3.3 ms for the full walk: such clusters walk full rows and skip the mirror.
        // The two walks do not build the same bits below the diagonal: an element is the fixed-point sum of (fp32 weight of the ROW's
        // rating) x (rating of the column), so the full walk forms G[j][i] from the weights of row j and the symmetric walk mirrors the
        // sum it formed from the weights of row i -- equal to ~1e-7, not to the bit.  A general-smoothing job keeps the symmetric walk
        // here, so that the plain full pass and the branch and bound (always symmetric) score one matrix and return the same rows bit
        // for bit; a Jelinek-Mercer job keeps the plan it always had.
        for (auto& p : plans) {
            const double deg2 = (size_t)p.c < in.cluster_deg2.size() ? (double)in.cluster_deg2[p.c] : (double)in.sum_deg2;
            if (!p.prune && !p.coop && p.half && tune.full_walk_sparse && !in.general_smoothing && deg2 < (double)p.Ic * (double)p.Ic) p.half = false;
        }
        if (n_pruned >= tune.panel_min_clusters)
            for (auto& p : plans)
                if (p.prune && !p.coop && use_pk && p.nch < 256 && p.nsub < 0xFFFF && p.Uc <= PLAN_STRAY_UCAP) {
                    p.panel = true;
                    p.half = false;      // a row's block maxima need the whole row
                    // (the item ids of the row kernel hold the chunk in 8 bits)
                    pick_chunks(p.Ic, std::min<int>(max_ch_lds, std::max<int>(tune.panel_max_ch, (int)round_up(ceil_div(p.Ic, 255), 256))), p.CH, p.nch);
                    // smaller clusters keep a wider panel: their survivors reach further down the popularity order (measured,
                    // ML-25M shape, ms per job with 4096 / 8192 columns: 50 clusters of 3250 users 124 / 141, 100 clusters of
                    // 1625 users 295 / 227, 200 clusters of 812 users 919 / 509 -- the difference is blocks behind the panel)
                    const int64_t want_cols = (int64_t)tune.panel_cols * (p.Uc < tune.panel_wide_below_users ? 2 : 1);
                    p.panel_cols = (int32_t)std::min<int64_t>(p.ldm, std::max<int64_t>(round_up(want_cols, 256), (int64_t)tune.seed_chunks * 256));
                    // (symmetric panel mode needs the head rows = the panel's columns: whole chunks of a width that divides the panel)
                    // Either the chunk width is re-picked so that it divides the panel, or -- where that would take too many rows out of
                    // the head (the rows with EXACT sub-block maxima; a tail row's bounds behind the panel are sums, and looser: Netflix
                    // shape in 50 clusters, chunks of 3584 columns: 7168 head rows; with 4096 head rows 3867 instead of 58 blocks survive
                    // behind the panel and the job takes 713 instead of 175 ms) -- the panel is widened to the chunks that cover it.
                    // (Widening from 1.25 x instead of 1.5 x the panel: 200 clusters of ML-25M shape 285 -> 299 ms, 25 clusters 59.8 -> 62.6 ms.)
                    const int64_t p_eff_chunks = std::min<int64_t>(ceil_div(p.panel_cols, p.CH) * (int64_t)p.CH, p.Ic);
                    if (tune.panel_sym && p.panel_cols % p.CH != 0 && 2 * p_eff_chunks > 3 * (int64_t)p.panel_cols && p_eff_chunks % 256 == 0 && p_eff_chunks < p.Ic)
                        p.panel_cols = (int32_t)p_eff_chunks;
                    if (tune.panel_sym && p.panel_cols % p.CH != 0) {
                        const int32_t lim = std::min<int>(max_ch_lds, std::max<int>(tune.panel_max_ch, (int)round_up(ceil_div(p.Ic, 255), 256)));
                        for (int32_t parts = 1; parts <= 8; parts++) {
                            const int32_t w = p.panel_cols / parts;
                            if (p.panel_cols % parts == 0 && w % 256 == 0 && w <= lim && ceil_div(p.Ic, w) < 256) { p.CH = w; p.nch = (int32_t)ceil_div(p.Ic, w); break; }
                        }
                    }
                    p.tail_chunks = (int32_t)ceil_div(p.panel_cols, p.CH);
                    p.p_eff = (int32_t)std::min<int64_t>((int64_t)p.tail_chunks * p.CH, p.Ic);
                    if (p.p_eff % 256 != 0 || p.tail_chunks >= p.nch) { p.p_eff = p.Ic; p.tail_chunks = 0; }   // one chunk, or a ragged one: no tail rows
                    p.tail_width = (int32_t)(p.ldb64 - p.p_eff / 64);
                    // (the chunks picked again under a forced FY_COOC_MAX_CH: the same limit as the first pick's)
                    if (p.nch >= 256) FY_PLAN_FAIL(FY_ERR_UNSUPPORTED, "cluster %d: %d items need %d column chunks (limit 255)", p.c, p.Ic, p.nch);
                }
    }
    const int64_t flat_budget = tune.flat_budget > 0 ? tune.flat_budget : (int64_t)std::min<uint64_t>(in.total_mem / 4, (uint64_t)std::max<int64_t>(ws, (int64_t)8 << 30));
    jp.flat_budget = flat_budget;
    {   // flat batch: the small unpruned clusters of a multi-cluster job, every kernel of their chain ONE launch for all of them
        // (FlatDesc, fy_rm2_kernels.hpp).  The matrices and score rows of the clusters of one batch are resident together; a job
        // whose clusters do not fit the budget takes several batches.
        int n_flat = 0;
        const bool can = tune.flat_batch && plans.size() > 1 && use_pk && tune.cooc_fx && !tune.cooc_f32 && !in.fx_bounds.empty() &&
                         in.number_of_recommendations <= PLAN_TOPN_LONG;
        for (auto& p : plans) {
            p.flat = false;
            if (!can || p.prune || p.coop || p.panel) continue;
            if (fx_exponent(&in.fx_bounds[3 * (size_t)p.c]) < 0) continue;
            if (flat_need(p) > flat_budget) continue;
            p.flat = true;
            n_flat++;
        }
        if (n_flat < 2)
            for (auto& p : plans) p.flat = false;
        for (auto& p : plans) p.psym = false;
        for (auto& p : plans)
            if (p.flat) p.half = false;      // (a mirror pass per cluster would be two more launches each)
    }
    bool any_panel = false;
    for (auto& p : plans) any_panel = any_panel || p.panel;
    jp.any_panel = any_panel;
    // Two phases for panel-mode jobs (round 3): the matrix panels of ALL clusters are built first, back to back on the main stream
    // (persistent row kernels that fill every CU's LDS gain nothing from running beside another cluster's), each into its own
    // buffers; then the clusters' light scoring kernels overlap on the lanes.  With one set of buffers per LANE (round 2) two lanes
    // were the optimum and mostly waited for each other's row kernels.  Needs every cluster's panel resident: 45 GB at 50 clusters
    // of ML-25M shape.
    int n_panel = 0;
    for (auto& p : plans)
        if (p.panel) n_panel++;
    // (more panels than fit a third of the HBM: the clusters are taken in GROUPS, each through all phases -- 100 clusters of ML-25M
    // shape keep 127 GB of panels)
    const bool two_phase = tune.panel_two_phase && n_panel >= 2;
    jp.two_phase = two_phase;
    std::vector<int>& group_of = jp.group_of;
    group_of.assign(plans.size(), 0);
    int n_groups = 1;
    if (two_phase) {
        const int64_t limit = tune.panel_group_bytes > 0 ? tune.panel_group_bytes : (int64_t)(in.total_mem / 3);
        int64_t in_group = 0;
        int g = 0;
        for (size_t pi = 0; pi < plans.size(); pi++) {
            const Plan& p = plans[pi];
            if (!p.panel) continue;
            const int64_t need = (int64_t)p.Ic * p.panel_cols * 3 + (int64_t)p.Ic * p.ldb64 * 7 + (int64_t)(p.b - p.a) * p.ldb64 * 7 + (int64_t)p.Ic * p.nch * 12;
            if (in_group > 0 && in_group + need > limit) { g++; in_group = 0; }
            in_group += need;
            group_of[pi] = g;
        }
        n_groups = g + 1;
    }
    jp.n_groups = n_groups;
    // Symmetric panel mode (two-phase jobs, batched fixed-point row kernels): G is symmetric, so (1) inside the panel's square
    // [0, p_eff)^2 the head rows are walked like the one-cluster job's -- only the columns behind the row, k_mirror_* fills the
    // rest -- and (2) the head rows are not walked over the tail columns at all: those co-ratings are the tail rows' with the head
    // columns, which the tail rows walk and STORE (Gp[j][i], j >= p_eff > i), and the only thing the head rows needed them for,
    // the maxima of their 64-column sub-blocks, are column maxima of the stored panel (k_panel_colmax).  Half the pair visits.
    if (two_phase && tune.panel_sym && tune.panel_multi_launch && use_pk && tune.cooc_fx && !tune.cooc_f32 && !in.fx_bounds.empty())
        for (auto& p : plans)
            p.psym = p.panel && p.tail_chunks > 0 && p.p_eff < p.Ic && p.p_eff == p.panel_cols && p.p_eff % 256 == 0 && p.a == p.sbase && p.b == p.sbase + p.Uc &&
                     fx_exponent(&in.fx_bounds[3 * (size_t)p.c]) >= 0;
    // (lanes: one-phase panel mode 2 -- more lanes only queue behind each other's row kernels; two-phase 8 -- only light kernels are left
    // on the lanes: measured at 50 clusters, ms per job: 2 lanes 98.0, 4: 95.9, 8: 93.1)
    const int want_lanes = tune.lanes_forced ? tune.lanes : (two_phase ? std::max(tune.lanes, 8) : (any_panel ? std::min(tune.lanes, tune.panel_lanes) : tune.lanes));
    const int NS = (int)std::min<size_t>(plans.size() > 1 ? (size_t)want_lanes : 1, plans.size());
    jp.NS = NS;
    {   // batch sizes, and the elements of the per-lane buffers (the largest need over the clusters a lane may get)
        size_t& is_el = jp.is_el;
        for (auto& p : plans)
            if (!p.flat) is_el = std::max(is_el, (size_t)p.Ic * p.nch);
        size_t &m_el = jp.m_el, &s_el = jp.s_el, &ov_el = jp.ov_el, &bm_el = jp.bm_el, &ub_el = jp.ub_el, &am_el = jp.am_el, &gp_el = jp.gp_el,
               &b64_el = jp.b64_el, &a64_el = jp.a64_el;
        for (auto& p : plans) {
            p.B = std::min<int64_t>(std::max<int64_t>(1, (ws / NS) / (p.ldm * 4)), p.b - p.a);
            // pruned clusters keep only the seed columns of a score row (the survivors' scores are packed, see below):
            // all users of the rank in one batch
            const int64_t seed_cols = (int64_t)std::min<int64_t>(ceil_div(p.Ic, 256), tune.seed_chunks) * 256;
            if (p.prune || p.flat) p.B = p.b - p.a;
            if (p.coop || p.flat) continue;   // allocate for themselves
            if (p.panel) {
                gp_el = std::max(gp_el, (size_t)p.Ic * p.panel_cols * 3 / 4 + 4);
                b64_el = std::max(b64_el, (size_t)p.Ic * p.ldb64 * 3 / 4 + 4);
                a64_el = std::max(a64_el, (size_t)p.ldb64);

                s_el = std::max(s_el, (size_t)(p.B * seed_cols));
                ov_el = std::max(ov_el, (size_t)p.B);
                ub_el = std::max(ub_el, (size_t)(p.B * p.ldb64));
                continue;
            }
            m_el = std::max(m_el, (size_t)(p.Ic * p.ldm));
            s_el = std::max(s_el, (size_t)(p.B * (p.prune ? seed_cols : p.ldm)));
            ov_el = std::max(ov_el, (size_t)p.B);
            if (p.prune) {
                bm_el = std::max(bm_el, (size_t)(p.Ic * p.ldb));
                ub_el = std::max(ub_el, (size_t)(p.B * p.ldb));
                am_el = std::max(am_el, (size_t)p.ldb);
            }
        }
    }
    for (auto& p : plans) jp.any_coop = jp.any_coop || p.coop;
    // (segment tables of the row kernel: which optional parts any cluster needs; their layout: fy_rm2_tables.hpp)
    for (auto& p : plans) {
        jp.any_tail = jp.any_tail || p.p_eff < p.Ic;
        jp.co_all = std::max(jp.co_all, (size_t)p.Uc * (p.nch + 1));
        jp.any_half = jp.any_half || p.half || p.p_eff < p.Ic;
        p.rect = tune.cooc_rect && p.half && !p.panel && !p.psym && !p.coop && !p.flat && p.nch > 1 && p.CH % 256 == 0;
    }
    return jp;
}

}  // namespace fy
