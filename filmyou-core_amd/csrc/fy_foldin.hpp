// fy_foldin.hpp -- fold-in of given profiles on standing factors (fy_foldin_*: fy_foldin.hip).
#pragma once
#include "fy_common.hpp"

namespace fy {

// one factor block in HBM: block 0 = the top level (items == nullptr: row = item id - 1), block 1 + c = parent cluster c of the refined level
struct FoldBlock {
    const double* W;            // m x k
    const double* C;            // k x k = W^T W
    const int32_t* items;       // m raw ids, ascending (row = position); nullptr for block 0
    const uint8_t* allowed;     // k flags, or nullptr: every column may win the argmax
    int32_t m, k;
};

fy_foldin* foldin_create(Context*, const fy_foldin_params*, const double* W, int location, const int32_t* count, int64_t n_count);
void foldin_add_level(fy_foldin*, int32_t n_parents, const int32_t* items_in_cluster, const int32_t* sub_clusters, const int32_t* item_raw,
                      const double* W_ragged, int32_t stride, const int32_t* count, int64_t n_count);
fy_foldin_result* foldin_assign(fy_foldin*, const fy_itemcf_profiles*, int32_t iterations, int32_t first_iteration, const double* h0, int32_t rank,
                                int32_t world);

}  // namespace fy

struct fy_foldin {
    fy::Context* ctx = nullptr;
    fy_foldin_params prm{};
    fy::DevBuf<double> W, C;                   // block 0
    fy::DevBuf<uint8_t> allowed0;              // k flags (has_mask0)
    bool has_mask0 = false;
    // the refined level (n_parents == 0: none)
    int32_t n_parents = 0, stride = 0;
    bool has_mask1 = false;
    std::vector<int32_t> m_c, k_c;             // per parent
    std::vector<int64_t> w_off, c_off, i_off, a_off;      // per parent + 1: offsets into W1 / C1 / items1 / allowed1
    fy::DevBuf<double> W1, C1;
    fy::DevBuf<int32_t> items1;
    fy::DevBuf<uint8_t> allowed1;
    fy::DevBuf<fy::FoldBlock> blocks;          // 1 + n_parents descriptors
};

struct fy_foldin_result {
    fy::Context* ctx = nullptr;
    int32_t k = 0;
    std::vector<int32_t> label, cluster, parent, status;
    std::vector<int64_t> sub_off;              // n + 1 (all 0 without a refined level)
    fy::DevBuf<double> H, H1;                  // n x k; ragged second-level factors
    fy_foldin_stats stats{};
};
