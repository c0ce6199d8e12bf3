// fy_itemsim_request.hpp -- the prepared item-similarity job (fy_itemsim_prepare: fy_itemsim.hip) and its request pass
// (fy_itemsim_rows: fy_itemsim_request.hip).
#pragma once
#include <memory>
#include <vector>

#include "fy_prep.hpp"
#include "fy_rm2.hpp"

// Everything the similarity job derives from the ratings and the parameters alone.  The job owns its buffers: nothing hangs on
// the fy_ratings object, which may be destroyed after prepare.  A request only reads it.
struct fy_itemsim_job {
    fy::Context* ctx = nullptr;
    fy_itemsim_params prm{};
    fy::Prepared P;                    // one-cluster structure after the input preparation (nnz == 0: nothing else is filled)
    int32_t CH = 0, nch = 0;           // column chunk of the request kernel (FY_ISIM_REQ_CHUNK at prepare) and chunks per row
    fy::DevBuf<int32_t> choff;         // [nU * (nch + 1)]: first entry of a user's CSR row inside every chunk (build_chunk_offsets)
    // per item in rank order
    fy::DevBuf<double> inv_norm;       // cosine: 1 / ||r_.i||; Pearson: 1 (NaN for a constant item); else unused
    fy::DevBuf<double> aux;            // the finishing measures' a_i (k_isim_rank_norms)
    fy::DevBuf<double> bound;          // >= |d| of every entry of the item's row: the fixed-point scale of the row
    // Pearson: per item in pair order, and the centred, normalised preference per CSR entry (0 on a constant item)
    fy::DevBuf<double> centre, cnorm, csr_w;
    // host: raw item ids ascending with their popularity rank, and per rank the sum of the raters' degrees
    std::vector<int32_t> raw_sorted, rank_of_sorted;
    std::vector<long long> walk;
    // Similarity rows kept for the item-CF request pass (fy_itemcf_recommend_prepared: fy_itemcf_request.hip), indexed by popularity
    // rank, in the layout k_icf_accumulate reads: allocated by the first such call, released by fy_itemsim_job_drop_rows.  A row is
    // valid only where state is 1 (written after the row is complete); fy_itemsim_rows neither reads nor fills it.
    struct RowStore {
        fy::DevBuf<int32_t> state;     // [nP] 1 = the row is here
        fy::DevBuf<int32_t> cnt;       // [nP] entries of the row
        fy::DevBuf<int32_t> start;     // [nP] j * K: the row_start of the accumulate kernel
        fy::DevBuf<int32_t> other;     // [nP * K] the other item as a column (popularity rank; -1 = no column)
        fy::DevBuf<float> sim;         // [nP * K]
        int64_t rows = 0;              // rows marked present
        bool allocated = false;
    } store;
};

namespace fy {
// the empty result of kind 1 over a job's structure, and its arrays sized for n rows (fy_itemsim.hip)
std::unique_ptr<fy_result> isim_empty_result(Context*, const Prepared&);
void isim_result_rows(fy_result*, int64_t n);
fy_itemsim_job* itemsim_prepare(Context*, const fy_itemsim_params*, const fy_ratings*);
fy_result* itemsim_rows(fy_itemsim_job*, const fy_itemsim_request*);
// rows of the given popularity ranks (device, ascending) -> cnt[n], other[n * K] (raw ids), sim[n * K]; returns the batches launched
int64_t itemsim_build_rank_rows(fy_itemsim_job*, const int32_t* rows, int64_t n, int32_t* cnt, int32_t* other, float* sim,
                                EventTimer& t_cooc, EventTimer& t_topn);
}  // namespace fy
