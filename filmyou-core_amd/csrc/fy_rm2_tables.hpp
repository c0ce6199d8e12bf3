// fy_rm2_tables.hpp -- the descriptors of the row kernel's walk tables (chunk offsets, packed CSR, the tail rows' block-compressed CSR,
// segment tables) and where a job's plan puts them (fy::layout_tables).  Host-only and pure like fy_rm2_plan.hpp: it builds with a
// plain C++17 compiler and is tested without a GPU (tests/test_rm2_tables_cpu.py).  The kernels that read the descriptors and the one
// host sequence that builds the tables: fy_cooc_tables.hpp.
#pragma once
#include "fy_rm2_plan.hpp"

namespace fy {

// the CSR side of one cluster: its chunk offsets (n_slots * (nch + 1) ints from co_off on), its range [f0, f1) of the packed CSR and,
// with has_tail, the block-compressed CSR of its tail rows (k_tail_blocks; two offsets per slot from co_tail_off on)
struct CsrDesc {
    int32_t slot_base, n_slots, CH, nch, f0, f1, p_eff, has_tail;
    int64_t co_off, co_tail_off;
};
inline CsrDesc csr_desc(int32_t slot_base, int32_t n_slots, int32_t CH, int32_t nch, int32_t f0 = 0, int32_t f1 = 0) {
    return CsrDesc{slot_base, n_slots, CH, nch, f0, f1, 0, 0, 0, 0};
}

// One segment table (fy_cooc.hpp): the CSC entries [q0, q0 + nq) of a cluster, each rater's CSR row cut at the cluster's chunk offsets
// (nch + 1 per slot from co_off on); its counts and prefixes are nch * (nq + 1) ints from cnt_off on.
// half (symmetric walk): the co-rating Gram is symmetric, so row i accumulates only the columns j > i and a mirror pass fills the
// lower triangle (k_mirror_*).  For the CSC entry (rater v, row i) the chunks in front of i's own chunk have no segments, and in i's
// chunk the rater's slice starts behind the position of i in the rater's CSR row -- at the 64-entry-aligned CSR position in front of
// (v, i), found once in the samples by k_seg_counts and re-used by k_seg_fill; the row kernel masks the entries at or before column i.
struct SegDesc {
    int32_t slot_base, q0, nq, nch, CH;
    int32_t half;
    // with half, the walk from the unpopular side (CoocArgs::half == 2): a cut entry has its segments in the chunks IN FRONT of its own
    // chunk (whole slices) and none behind it; the own chunk is cut as ever
    int32_t rect;
    // column-panel mode: with half, only the rows in front of sym_rows are cut (0 = all rows), and the rows from lim_from on have
    // segments only in their first lim_chunks chunks (0 = off) -- rows and chunks the item list never names (tail rows behind the
    // panel's chunks; symmetric panel mode: every row)
    int32_t sym_rows, lim_from, lim_chunks;
    int32_t only_from;      // tail-row tables: the entries of the rows in front of only_from get no segments (0 = all rows)
    int32_t pad;
    int64_t co_off, cnt_off;
};
// a table of its own (one cluster, or one rank's rows of a cluster): full walk, or the symmetric one
inline SegDesc seg_desc(int32_t slot_base, int32_t q0, int32_t nq, int32_t nch, int32_t CH = 0, bool half = false) {
    return SegDesc{slot_base, q0, nq, nch, CH, half ? 1 : 0, 0, 0, 0, 0, 0, 0, 0, 0};
}
inline int64_t seg_desc_counts(const SegDesc& d) { return (int64_t)d.nch * ((int64_t)d.nq + 1); }

// The tables of every planned cluster as ranges of shared arrays.  csr[plan] for every plan (a cooperative plan gets its packed-CSR
// range and nothing else: its ranks build the tables of their own rows); seg = the main tables of the other plans in plan order, then
// the tail tables (p_eff < Ic: one chunk over the block-compressed CSR) -- the two read different chunk offsets, so they are two groups.
struct TableLayout {
    std::vector<CsrDesc> csr;
    std::vector<SegDesc> seg;
    std::vector<int32_t> main_of, tail_of;      // [plan] -> index in seg, -1 = none
    size_t n_main = 0;
    int64_t co_total = 0, co_tail_total = 0, cnt_total = 0;
};
inline TableLayout layout_tables(const std::vector<Plan>& plans, const std::vector<int32_t>& csr_range) {
    TableLayout L;
    const size_t np = plans.size();
    L.csr.resize(np);
    L.main_of.assign(np, -1);
    L.tail_of.assign(np, -1);
    for (size_t pi = 0; pi < np; pi++) {
        const Plan& p = plans[pi];
        const bool tail = !p.coop && p.p_eff < p.Ic;
        L.csr[pi] = CsrDesc{p.sbase, p.coop ? 0 : p.Uc, p.CH, p.nch, csr_range[2 * pi], csr_range[2 * pi + 1], p.p_eff, tail ? 1 : 0, L.co_total, L.co_tail_total};
        if (p.coop) continue;
        // panel mode: the tail rows are walked over their first tail_chunks chunks only; symmetric panel mode: so are the head rows,
        // and those are cut -- rows and chunks the item list never names get no segments
        SegDesc m = seg_desc(p.sbase, p.q0, p.nq, p.nch, p.CH, p.half || p.psym);
        m.rect = (m.half && p.rect) ? 1 : 0;
        m.sym_rows = p.psym ? p.p_eff : 0;
        m.lim_from = p.psym ? 0 : p.p_eff;
        m.lim_chunks = (p.panel && p.tail_chunks > 0 && tail) ? p.tail_chunks : 0;
        m.co_off = L.co_total;
        m.cnt_off = L.cnt_total;
        L.main_of[pi] = (int32_t)L.seg.size();
        L.seg.push_back(m);
        L.cnt_total += seg_desc_counts(m);
        L.co_total += (int64_t)p.Uc * (p.nch + 1);
        if (tail) L.co_tail_total += 2 * (int64_t)p.Uc;
    }
    L.n_main = L.seg.size();
    for (size_t pi = 0; pi < np; pi++) {
        if (!L.csr[pi].has_tail) continue;
        const Plan& p = plans[pi];
        SegDesc t = seg_desc(p.sbase, p.q0, p.nq, 1);
        t.only_from = p.p_eff;
        t.co_off = L.csr[pi].co_tail_off;
        t.cnt_off = L.cnt_total;
        L.tail_of[pi] = (int32_t)L.seg.size();
        L.seg.push_back(t);
        L.cnt_total += seg_desc_counts(t);
    }
    if (L.cnt_total + 1 >= (int64_t)0x7FFFFFF0)
        FY_PLAN_FAIL(FY_ERR_UNSUPPORTED, "segment tables of %zu clusters need %lld prefix entries (limit 2^31)", np, (long long)L.cnt_total);
    return L;
}

}  // namespace fy
