// fy_rm2_launch.hpp -- which instantiation of a kernel family a Tuning switch picks, and the one launcher of every family.
// NOT a standalone header: one section of fy_rm2.hip's translation unit (included inside `namespace fy`, behind the kernels).
// Every variant switch (FY_SCORE_WALK, FY_COOC_EPI, FY_TOPN_SEED_XL) is a template argument of its kernels; the selectors below are the
// only places that name the instantiations, the launchers the only functions that launch them.
#pragma once

// ---- selectors.  The nine leading parameters are ScoreArgs members passed on their own (scalar registers from the start: fy_rm2_kernels.hpp)
using ScoreKernel = void (*)(const float*, const float*, const int32_t*, const int32_t*, const float*, const float*, const double*, const int32_t*,
                             float*, ScoreArgs);
using CoocKernel = void (*)(CoocArgs, MEpilogue, int, int*);
using CoocMultiKernel = void (*)(const CoocLaunch*, int*);

// (the fp32 rows have one walk: `walk` picks among the 24-bit instantiations only)
static ScoreKernel score_kernel(bool pack24, int walk) {
    if (!pack24) return k_score<4, false, 8>;
    return walk ? k_score<4, true, 8, 1> : k_score<4, true, 8, 0>;
}
static auto score_multi_kernel(bool pack24, int walk) {
    if (!pack24) return k_score_multi<4, false, 8>;
    return walk ? k_score_multi<4, true, 8, 1> : k_score_multi<4, true, 8, 0>;
}
static ScoreKernel score_sup_kernel(int walk) { return walk ? k_score_sup<1> : k_score_sup<0>; }
static auto score_blocks_kernel(int walk) { return walk ? k_score_blocks<8, 1> : k_score_blocks<8, 0>; }

// lp2 = the size of the seed sort (a power of two, 64 .. 1024: lp2 / 64 keys per lane)
static auto topn_seed_kernel(int lp2, int xl) {
    static void (*const K[5][2])(TopNArgs, int32_t, int32_t*) = {{k_topn_seed<1, 0>, k_topn_seed<1, 1>}, {k_topn_seed<2, 0>, k_topn_seed<2, 1>}, {k_topn_seed<4, 0>, k_topn_seed<4, 1>},
                                                                 {k_topn_seed<8, 0>, k_topn_seed<8, 1>}, {k_topn_seed<16, 0>, k_topn_seed<16, 1>}};
    return K[lp2 <= 64 ? 0 : lp2 == 128 ? 1 : lp2 == 256 ? 2 : lp2 == 512 ? 3 : 4][xl ? 1 : 0];
}

// Every instantiation of the row kernel the library launches, [epi] = Tuning::cooc_epi.  cooc_rm2_kernel chooses from this table and
// cooc_rm2_allow_lds walks it: an instantiation that can be launched has its LDS attribute.
enum CoocAcc { COOC_ACC_U64, COOC_ACC_U32, COOC_ACC_F64, COOC_ACC_F32 };
struct CoocVariant { bool pk; CoocAcc acc; int role; CoocKernel fn[2]; };
static const CoocVariant COOC_RM2_VARIANTS[] = {
    {true, COOC_ACC_U64, 0, {k_cooc_rm2<true, unsigned long long, 0, 0>, k_cooc_rm2<true, unsigned long long, 0, 1>}},
    {true, COOC_ACC_U64, 1, {k_cooc_rm2<true, unsigned long long, 1, 0>, k_cooc_rm2<true, unsigned long long, 1, 1>}},
    {true, COOC_ACC_U32, 0, {k_cooc_rm2<true, uint32_t, 0, 0>, k_cooc_rm2<true, uint32_t, 0, 1>}},
    {true, COOC_ACC_F64, 0, {k_cooc_rm2<true, double, 0, 0>, k_cooc_rm2<true, double, 0, 1>}},
    {false, COOC_ACC_F64, 0, {k_cooc_rm2<false, double, 0, 0>, k_cooc_rm2<false, double, 0, 1>}},
    {true, COOC_ACC_F32, 0, {k_cooc_rm2<true, float, 0, 0>, k_cooc_rm2<true, float, 0, 1>}},
    {false, COOC_ACC_F32, 0, {k_cooc_rm2<false, float, 0, 0>, k_cooc_rm2<false, float, 0, 1>}},
};
// the batched launches: fixed-point packed walk only, [role][epi]
static const CoocMultiKernel COOC_RM2_MULTI[2][2] = {
    {k_cooc_rm2_multi<true, unsigned long long, 0, 0>, k_cooc_rm2_multi<true, unsigned long long, 0, 1>},
    {k_cooc_rm2_multi<true, unsigned long long, 1, 0>, k_cooc_rm2_multi<true, unsigned long long, 1, 1>},
};
static CoocKernel cooc_rm2_kernel(bool pk, CoocAcc acc, int role, int epi) {
    for (const CoocVariant& v : COOC_RM2_VARIANTS)
        if (v.pk == pk && v.acc == acc && v.role == role) return v.fn[epi ? 1 : 0];
    FY_FAIL(FY_ERR_STATE, "internal: no row kernel for packed %d, accumulator %d, role %d", (int)pk, (int)acc, role);
}
static CoocMultiKernel cooc_rm2_multi_kernel(int role, int epi) { return COOC_RM2_MULTI[role ? 1 : 0][epi ? 1 : 0]; }

static void cooc_rm2_allow_lds(int epi) {    // (Tuning::cooc_epi: the instantiations this context launches)
    const int bytes = 160 * 1024 - 256;     // everything but the kernel's few static words
    for (const CoocVariant& v : COOC_RM2_VARIANTS)
        FY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(v.fn[epi ? 1 : 0]), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    for (int role = 0; role < 2; role++)
        FY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(cooc_rm2_multi_kernel(role, epi)), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
}

// ---- launchers
static void launch_score(ScoreKernel k, int grid, hipStream_t st, const ScoreArgs& A) {
    k<<<grid, 256, 0, st>>>(A.M, A.a_rank, A.rb_off, A.csr_idx, A.csr_e, A.csr_q, A.pvpi, A.n_out, A.S, A);
    FY_KERNEL_CHECK();
}

// one top-N pass over n_rows score rows: k_topn_long (`long_list`: lists of more than TOPN_LONG entries, or a seed wider than TOPN_SAMPLE; top_n
// sizes its candidate buffer) or k_topn_fast.  On its own this is the seed phase of the branch and bound (TopNArgs::mode 1: tau and
// the speculative lists, nothing is flagged).
static void launch_topn_pass(hipStream_t st, const TopNArgs& TA, int32_t n_rows, int32_t* overflow, int32_t* any_overflow, int force_select, bool long_list,
                             int top_n) {
    if (long_list) k_topn_long<<<n_rows, 256, (size_t)fy_topn_long_cap(top_n) * 8, st>>>(TA, overflow, any_overflow, force_select, fy_topn_long_cap(top_n));
    else k_topn_fast<<<n_rows, 256, 0, st>>>(TA, overflow, any_overflow, force_select);
    FY_KERNEL_CHECK();
}
// the lists of n_rows rows: flag reset, the pass, the radix select for the rows the pass flagged (n_selected counts them, or null)
static void launch_topn(Context* ctx, hipStream_t st, const TopNArgs& TA, int32_t n_rows, int32_t* overflow, int32_t* any_overflow, int force_select, bool long_list,
                        int top_n, unsigned long long* n_selected) {
    FY_HIP(hipMemsetAsync(any_overflow, 0, sizeof(int32_t), st));
    launch_topn_pass(st, TA, n_rows, overflow, any_overflow, force_select, long_list, top_n);
    k_topn_select<<<fy_topn_select_grid(n_rows, ctx->num_cus), 256, 0, st>>>(TA, overflow, any_overflow, n_rows, n_selected);
    FY_KERNEL_CHECK();
}

// launch shape of the RM2 row kernel: as many workgroups per CU as the LDS accumulators allow (fp32: two for ML-25M's 19 712-column chunks), 2048 threads
// per CU at most
struct CoocShape { int block, max_grid; };
static CoocShape cooc_launch_shape(size_t lds_bytes, const Tuning& tune, int num_cus) {
    const int by_lds = (int)std::max<size_t>(1, (160 * 1024 - 512) / (lds_bytes + 64));
    int block = tune.cooc_block;
    if (!block) block = by_lds >= 4 ? 256 : (by_lds >= 2 ? 512 : 1024);
    return CoocShape{block, num_cus * std::max(1, std::min(by_lds, 2048 / block))};
}
// items per atomic of the row kernel's work counter: 8 where an item is short (fewer than ~12 000 co-rating contributions, i.e.
// < 256 segments on average; `visits` = the cluster's sum of n_u^2, an upper bound of the launch's contributions), else 1
static int cooc_item_grab(int64_t visits, int64_t n_items) { return n_items > 0 && visits / n_items < 12000 ? 8 : 1; }

// The accumulators: 64-bit fixed point in the packed walk with a scale (32-bit where the caller has shown the sums fit:
// CoocArgs::acc32), else fp64; FY_COOC_F32=1 (measurement only) takes fp32 in every case.  ME.ceil24 (the tail rows' bound
// launch) names the fixed-point instantiation by its role.
static void launch_cooc_rm2(Context* ctx, const Tuning& tune, bool use_pk, const CoocArgs& CA_, const MEpilogue& ME, int n_items,
                            int32_t* counter, hipStream_t st) {
    if (n_items <= 0) return;
    CoocArgs CA = CA_;
    CA.acc_quarter = tune.cooc_planes ? cooc_lds_columns(CA.CH) / 4 : 0;
    const bool fixed = use_pk && CA.fx_scale > 0.0 && !tune.cooc_f32;
    const CoocAcc acc = fixed ? (CA.acc32 ? COOC_ACC_U32 : COOC_ACC_U64) : (tune.cooc_f32 ? COOC_ACC_F32 : COOC_ACC_F64);
    const size_t lds = (size_t)cooc_lds_columns(CA.CH) * ((acc == COOC_ACC_F32 || acc == COOC_ACC_U32) ? 4 : 8);
    const CoocShape sh = cooc_launch_shape(lds, tune, ctx->num_cus);
    const int grid = std::min(n_items, sh.max_grid);
    cooc_rm2_kernel(use_pk, acc, acc == COOC_ACC_U64 && ME.ceil24 ? 1 : 0, tune.cooc_epi)<<<grid, sh.block, lds, st>>>(CA, ME, n_items, counter);
    FY_KERNEL_CHECK();
}

// one launch for the row kernels of several clusters (two-phase panel mode, flat batches; fixed-point packed walk only): `L` = one
// CoocLaunch per cluster on the host, uploaded here; the launch shape (workgroup size, LDS) is that of the widest chunk among them
static void launch_cooc_rm2_multi(Context* ctx, const Tuning& tune, std::vector<CoocLaunch>& L, bool tail_role, DevBuf<CoocLaunch>& d_launch,
                                  DevBuf<int32_t>& d_counters, hipStream_t st, bool item_lists = false /* fill the item lists first */) {
    if (L.empty()) return;
    int max_chp = 0, max_items = 0, max_list = 0;
    for (size_t k = 0; k < L.size(); k++)      // (a null operand here is a fault on the GPU a moment later)
        if (!L[k].A.item_seg || !L[k].A.item_id || !L[k].E.M || !L[k].A.seg || !L[k].A.seg_ptr || (L[k].E.panel_cols && !L[k].E.Bmax64))
            FY_FAIL(FY_ERR_STATE, "internal: launch %zu of %zu of a batched row kernel has a null operand (item_seg %p item_id %p M %p seg %p ptr %p Bmax64 %p)", k, L.size(),
                    (const void*)L[k].A.item_seg, (const void*)L[k].A.item_id, (const void*)L[k].E.M, (const void*)L[k].A.seg, (const void*)L[k].A.seg_ptr, (const void*)L[k].E.Bmax64);
    for (auto& x : L) {
        x.A.acc_quarter = tune.cooc_planes ? cooc_lds_columns(x.A.CH) / 4 : 0;
        max_chp = std::max(max_chp, cooc_lds_columns(x.A.CH));
        max_items = std::max(max_items, x.n_items);
        max_list = std::max(max_list, x.A.nrows * x.A.nch);
    }
    const size_t lds = (size_t)max_chp * 8;
    const CoocShape sh = cooc_launch_shape(lds, tune, ctx->num_cus);
    const int gx = std::max(1, std::min(max_items, sh.max_grid));
    d_launch.alloc(ctx, L.size());
    d_counters.alloc(ctx, L.size());
    FY_HIP(hipMemcpyAsync(d_launch.get(), L.data(), L.size() * sizeof(CoocLaunch), hipMemcpyHostToDevice, st));
    FY_HIP(hipMemsetAsync(d_counters.get(), 0, L.size() * sizeof(int32_t), st));
    if (item_lists) {
        k_item_list_multi<<<dim3((unsigned)std::max(1, std::min(grid_for(max_list), 4096)), (unsigned)L.size()), 256, 0, st>>>(d_launch.get());
        FY_KERNEL_CHECK();
    }
    cooc_rm2_multi_kernel(tail_role, tune.cooc_epi)<<<dim3((unsigned)gx, (unsigned)L.size()), sh.block, lds, st>>>(d_launch.get(), d_counters.get());
    FY_KERNEL_CHECK();
}
