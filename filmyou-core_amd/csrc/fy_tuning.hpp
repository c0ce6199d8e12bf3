// fy_tuning.hpp -- the launch-shape knobs and the two integer helpers the host-side planning shares with the HIP translation units.
// Host-only: no HIP header, so that the planning (fy_rm2_plan.hpp) builds with a plain C++17 compiler.
#pragma once
#include <cstdint>

namespace fy {

// ---------------------------------------------------------------- launch-shape knobs
// Defaults are the production values.  The environment overrides (FY_*) are TEST AND MEASUREMENT HOOKS: each
// one forces a path that the default heuristics would pick only at a larger size, so that the parity tests can drive every
// path at a size the oracle finishes; none of them changes a result beyond the summation order.  The environment is read ONCE,
// when the context is created (load_tuning_from_env, fy_api.hip; fy_context_reload_tuning reads it again) -- no job calls getenv.
struct Tuning {
    int force_select = 0;              // route every user through k_topn_select
    int pack24 = 1;                    // M rows as 24-bit floats (3 bytes per element): -25 % of the dominant traffic
    int pack24_min_items = 4096;       // ... for clusters with at least this many items
    int max_slices = 65536;            // user slices (workgroups) per column chunk
    int users_per_wave = 16;           // users a wave of the scoring kernel walks for one column chunk
    int64_t workspace_default = (int64_t)16 << 30;   // score scratch per batch of users
    int lanes = 4;                     // HIP streams the clusters of one job are spread over
    bool lanes_forced = false;         // FY_LANES given: panel mode does not lower it
    int prune = 1;                     // branch and bound over 256-column candidate blocks
    int prune_min_items = 8192;
    int seed_chunks = 0;               // 256-column chunks scored exactly before the bound pass (the most popular candidates);
                                       // 0 = from the list length: ~5 N columns (N = 50: one chunk, N = 100: two), at most four
    int cooc_block = 0;                // force the row kernel's workgroup size
    int cooc_max_ch = 19968;           // LDS accumulators of the row kernel: 156 KiB of 64-bit words of the 160 KiB LDS (ML-25M shape: three
                                       // column chunks instead of four, 19.7 -> 17.8 ms; smaller forces more chunks)
    bool cooc_max_ch_forced = false;   // FY_COOC_MAX_CH given (the item-similarity build has its own default)
    int sup_bounds = 1;                // FY_SUP_BOUNDS: one-cluster pruned jobs bound over <= 64 super-blocks inside the seed pass (0: a bound chunk per user over all blocks)
    int prep_packed = 1;               // FY_PREP_PACKED: fp16-exact scores ride in the low 16 bits of the prep's sort keys, the three nnz-sized sorts move keys alone
    int overlap_values = 1;            // FY_OVERLAP_VALUES: the per-rating values of the scoring kernels are computed on a side stream beside the one-cluster job's row kernel
    int shard_prep = 1;                // FY_SHARD_PREP: several ranks, clusters >= ranks: a rank preps its own clusters' ratings alone (fy_prep.hpp)
    int full_walk_sparse = 1;          // FY_FULL_WALK_SPARSE: unpruned clusters whose matrix has more elements than the cluster has pair visits walk full rows (no mirror pass)
    int refine = 1;                    // FY_REFINE: list rows whose score nearly cancels are scored again in fp64 from fp32 head rows (k_refine_rows)
    float refine_c = 2.0f;             // FY_REFINE_C: ... those with |score| < refine_c * sqrt(ratings of the user)
    int lazy_mirror = 1;               // FY_LAZY_MIRROR: pruned one-cluster jobs mirror only the column blocks somebody reads (0: the whole lower triangle)
    int seed_forced = 0;               // FY_SEED_CHUNKS given: prune whatever the list length
    int coop = 1;                      // cooperative scoring of clusters that span all ranks (needs fy_collectives)
    int coop_force = 0;                // cooperative path also with world == 1 (identity collectives)
    int cooc_pk = 1;                   // packed 4-byte CSR entries for the row kernel when the ratings are fp16-exact
    int cooc_f32 = 0;                  // row kernel accumulators in fp32 (ds_add_f32): MEASUREMENT ONLY -- 4x slower, see fy_cooc.hpp
    int cooc_half = 1;                 // symmetric walk (upper triangle + mirror pass) for clusters with packed rows
    int cooc_rect = 1;                 // FY_COOC_RECT=0: the symmetric walk of a row covers its own chunk and the chunks BEHIND it (before DESIGN.md section 7g)
                                       // instead of its own chunk and the whole chunks IN FRONT of it; last-bit differences in the off-diagonal chunk rectangles
    int cooc_fx = 1;                   // fixed-point (ds_add_u64) accumulation in the packed walk
    int panel_min_clusters = 4;        // column-panel mode when at least this many clusters of the rank are pruned ones
    int prune_min_users = 600;         // clusters with fewer users take the plain full pass
    int panel_wide_below_users = 2500; // panel mode: clusters with fewer users keep twice the panel columns
    int panel_cols = 4096;             // columns of a row kept in panel mode (the seed columns and the popular blocks)
    bool cooc_planes = true;           // FY_COOC_PLANES=0: linear accumulator layout (measurement only)
    int score_heavy = 512;             // users with more ratings are walked by a whole workgroup of the scoring kernel (0 = off)
    int score_walk = 1;                // FY_SCORE_WALK=0: the 24-bit scoring kernels walk every batch the first way (v_readlane triplets, a mask test per row); same bits, measurement and parity tests only
    int cooc_epi = 1;                  // FY_COOC_EPI=0: the row kernel's epilogue as before DESIGN.md section 7f (four columns per lane everywhere, block maxima by __shfl_xor); same bits, measurement and parity tests only
    int topn_seed_xl = 1;              // FY_TOPN_SEED_XL=0: k_topn_seed's register sort exchanges lanes by __shfl_xor (ds_bpermute) instead of DPP / v_permlane swaps; same lists, measurement and parity tests only
    bool panel_repair = true;          // FY_PANEL_REPAIR=0: measurement only
    int panel_lanes = 2;               // job lanes when clusters run in panel mode (measured, 50 clusters: 1 lane 300 ms, 2: 213, 3: 230, 4: 240)
    int64_t flat_budget = 0;           // FY_FLAT_BUDGET_MB: bytes of matrices + score rows one flat batch may hold (0 = a quarter of the HBM, at most the workspace)
    int64_t panel_group_bytes = 0;     // FY_PANEL_GROUP_MB: bytes of panels + scoring scratch one group of panel-mode clusters may hold (0 = a third of the HBM)
    int debug_sync = 0;                // FY_DEBUG_SYNC=1: multi-cluster jobs drain the device after every step of a cluster and say on stderr where they are; 2: only the wall clock of the phases (drains the device at the phase ends)
    bool panel_sym = true;             // FY_PANEL_SYM=0: panel mode walks the head rows over all their chunks (round 2) instead of symmetrically over the panel's
    bool flat_batch = true;            // FY_FLAT=0: small unpruned clusters one after the other on the lanes (round 2) instead of one launch per kernel
    bool panel_multi_launch = true;    // FY_PANEL_MULTI_LAUNCH=0: one row-kernel launch per cluster also in two-phase panel mode
    bool panel_two_phase = true;       // FY_PANEL_TWO_PHASE=0: every cluster start to end on its lane (round 2)
    int panel_max_ch = 4096;           // chunk width of the row kernel in panel mode: five workgroups per CU (measured, 50 clusters, row kernel ms: 8192 -> 67, 6144 -> 54, 4096 -> 46)
    double max_surv_frac = 0.25;       // a pruned batch whose surviving blocks exceed this fraction falls back to the full pass
    // restricted RM2 pass (fy_rm2_request.hip)
    double req_full_share = 1.0;       // FY_REQ_FULL_SHARE: a cluster of which more than this share of the users is asked for is scored by the full pass and the
                                       // unrequested rows are dropped (0 = every touched cluster, >= 1 = never).  Not measured yet ("RM2 on
                                       // request"), so the default never falls back; ONE cluster that does costs the rank's whole full job
    int req_chunk = 8192;              // FY_REQ_CHUNK: columns (64-bit LDS accumulators) a workgroup of the slab build owns
    // RM1 estimator (fy_rm1.hip); neither changes a bit of a result
    int rm1_nbr_chunk = 512;           // FY_RM1_NBR_CHUNK: neighbours a workgroup of k_rm1_loglik takes (its four waves share the user's LDS bitmask)
    int rm1_col_chunk = 1024;          // FY_RM1_COL_CHUNK: candidate columns a workgroup of k_rm1_score owns (a lane walks one column at a time)
    // ratings update (fy_ratings_update.hip)
    int upd_lds_keys = 4096;           // FY_UPD_LDS_KEYS: a batch of at most this many distinct keys is searched in LDS (32 KiB of keys beside the 32 KiB
                                       // user bitmap: two workgroups per CU), a larger one in global memory (0 = always); at most 8192
    // item-item similarity build (fy_itemsim.hip)
    int isim_heavy = 4096;             // row-at-a-time kernel: raters above which a row is split by column chunk
    int isim_gram = -1;                // symmetric Gram + band sweep: -1 = by size (cosine, >= isim_gram_min_items items), 0 = never, 1 = whenever possible
    int isim_gram_min_items = 4096;
    int isim_capg = 2040;              // candidates a row of the band sweep may collect before it is redone exactly (<= 2040: k_isim_finish sorts them in LDS)
    int isim_piece = 4096;             // columns per piece of the band sweep (measured, ML-25M shape, build ms: 2048 11.90, 4096 11.90, 8192 12.2, 16384 12.0, 32768 12.5, 65536 14.1)
    int isim_acc32 = 1;                // 32-bit fixed-point accumulators in the symmetric build's walk when the products are exact integers
    // item similarity on request (fy_itemsim_request.hip); neither changes a result
    int isim_req_chunk = 8192;         // FY_ISIM_REQ_CHUNK: most columns (64-bit LDS accumulators) a workgroup of the row kernel owns (a row's chunks are balanced); read at fy_itemsim_prepare,
                                       // which keeps the row offsets for this width
    int isim_req_rows = 0;             // FY_ISIM_REQ_ROWS: rows per batch of a request (0 = as many as the partial lists of workspace_default hold)
    // item-CF estimates for named pairs (fy_itemcf_estimate.hip); changes no result
    int icf_est_chunk = 256;           // FY_ICF_EST_CHUNK: most distinct targets of one user a wave of the estimate kernel holds in LDS (28 B each; four
                                       // waves a workgroup: 28 KiB at 256); at most 512
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t round_up(int64_t a, int64_t b) { return ceil_div(a, b) * b; }

}  // namespace fy
