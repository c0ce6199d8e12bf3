// fy_refine.hpp -- what SubClusterMappingJob leaves in HBM, and the result object of fy_cluster_refine (fy_refine.hip).
#pragma once
#include "fy_common.hpp"

namespace fy {

// Users and items of every parent cluster under new, dense "row" numbers: cluster-major, inside a cluster ascending raw id
// (new id of the reference = row - start[cluster] + 1), and the kept ratings remapped to those rows, sorted both ways.
struct SubMap {
    Context* ctx = nullptr;
    int32_t K = 0;
    int32_t n_tab = 0;      // entries of the raw-user tables: 1 + the largest user id of the map or the ratings
    int32_t I = 0;          // 1 + the largest item id of the ratings
    int32_t n_users = 0, n_items = 0;      // sum of n_c, sum of m_c
    int64_t nnz = 0;                       // kept ratings
    int64_t launches = 0;
    std::vector<int32_t> ustart, istart;   // K + 1: first row of every cluster
    DevBuf<int32_t> cl_of_raw, row_of_raw;                 // n_tab: cluster of a raw user id (-1: not in the map), its row (-1)
    DevBuf<int32_t> user_raw, user_cl, d_ustart;           // n_users, n_users, K + 1
    DevBuf<int32_t> ipos;                                  // K x I + 1: row of (cluster, raw item); present iff ipos[x + 1] > ipos[x]
    DevBuf<int32_t> item_raw, item_cl, d_istart;           // n_items, n_items, K + 1
    DevBuf<uint64_t> ku, ki;                               // sorted (user row << 32 | item row) and (item row << 32 | user row)
    DevBuf<float> vu, vi;
    DevBuf<int32_t> uptr, iptr;                            // n_users + 1, n_items + 1
};

void build_submap(Context* ctx, const fy_ratings* R, int32_t K, int64_t n_map, const int32_t* map_user, const int32_t* map_cluster, SubMap& out);
fy_refined* cluster_refine(Context* ctx, const fy_refine_params* prm, const fy_ratings* R, int64_t n_map, const int32_t* map_user,
                           const int32_t* map_cluster, const double* H0, const double* W0);

}  // namespace fy

struct fy_refined {
    fy::Context* ctx = nullptr;
    std::vector<int32_t> user, cluster, count;      // the refined `clustering` and `clusteringCount`
    std::vector<int32_t> users_in_cluster, items_in_cluster, k;   // per parent cluster
    int32_t stride = 0;
    fy::DevBuf<double> H, W;      // the final factors, ragged (cluster after cluster), in HBM
    int64_t h_size = 0, w_size = 0;
    fy_refine_stats stats{};
};
