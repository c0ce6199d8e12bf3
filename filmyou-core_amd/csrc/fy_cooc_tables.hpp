// fy_cooc_tables.hpp -- the tables every co-rating walk reads (chunk offsets, packed CSR, block-compressed CSR of the tail rows, segment
// tables): ONE set of kernels driven by table descriptors (fy_rm2_tables.hpp; blockIdx.y = table) and ONE host sequence that builds
// any number of tables at once.  One table is the case of one descriptor.
// NOT a standalone header: one section of fy_rm2.hip's translation unit, inside namespace fy (like fy_rm2_launch.hpp); the host
// functions are declared in fy_cooc.hpp for the other translation units.
#pragma once

// packed CSR of one cluster for the row kernel (fy_cooc.hpp): column index relative to its chunk | fp16 raw rating
__device__ __forceinline__ void pack_csr_body(int32_t f0, int32_t f1, int32_t CH, const int32_t* __restrict__ csr_idx, const float* __restrict__ csr_r,
                                              uint32_t* __restrict__ pk) {
    for (int64_t f = f0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < f1; f += (int64_t)gridDim.x * blockDim.x)
        pk[f] = (uint32_t)(csr_idx[f] % CH) | ((uint32_t)__half_as_ushort(__float2half(csr_r[f])) << 16);
}
__global__ void k_pack_csr(const CsrDesc* __restrict__ D, const int32_t* __restrict__ csr_idx, const float* __restrict__ csr_r, uint32_t* __restrict__ pk) {
    const CsrDesc d = D[blockIdx.y];
    pack_csr_body(d.f0, d.f1, d.CH, csr_idx, csr_r, pk);
}

// Column-panel mode, tail rows (rows >= p_eff, few raters each): their co-ratings with the columns behind p_eff are needed only
// as upper bounds of the 64-column block maxima.  For a row i and a block B
//     max_{j in B} sum_v x_vi x_vj  <=  sum_v x_vi max_{j in B} x_vj ,
// and the right-hand side is the row kernel's own sum over a CSR compressed to ONE entry per (rater, block): the block index
// relative to p_eff | the largest raw rating of the rater in the block, in the packed format of k_pack_csr.  With 2-17 raters
// per tail row the sum of maxima is within ~14 % of the exact maximum (measured at ML-25M shape in 50 clusters: 1088
// surviving blocks instead of 1080), a row needs ONE item with (I_c - p_eff) / 64 accumulators instead of one item per
// 8192-column chunk, and no matrix element behind the panel is ever formed.
// The user's compressed entries are written in place of the first entries of its CSR range (y_pk is as long as the CSR),
// co2[2 k] / co2[2 k + 1] = their range: the "chunk offsets" of a one-chunk segment table.
__device__ __forceinline__ void tail_blocks_body(int32_t slot_base, int32_t n_slots, int32_t p_eff, const int32_t* __restrict__ rowptr,
                                                const int32_t* __restrict__ csr_idx, const float* __restrict__ csr_r, uint32_t* __restrict__ y_pk,
                                                int32_t* __restrict__ co2) {
    // One workgroup per user: the entries behind p_eff are a suffix of the row (found by a binary search), its 64-entry pieces
    // are dealt to the four waves; a piece looks one entry back for the block of its predecessor and takes its output slots
    // from an LDS counter (the order of a user's compressed entries does not matter: the sums they enter are integer sums).
    __shared__ int sh_count;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int32_t k = blockIdx.x; k < n_slots; k += gridDim.x) {      // block-uniform
        const int32_t base = rowptr[slot_base + k], end = rowptr[slot_base + k + 1];
        int32_t lo = base, hi = end;                                  // first entry with column >= p_eff
        while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (csr_idx[mid] < p_eff) lo = mid + 1; else hi = mid; }
        const int32_t first = lo;
        if (threadIdx.x == 0) sh_count = 0;
        __syncthreads();
        for (int32_t f0 = first + wave * 64; f0 < end; f0 += 4 * 64) {   // wave-uniform
            const int32_t f = f0 + lane;
            const int blk = f < end ? (csr_idx[f] - p_eff) >> 6 : -1;
            int prev = __shfl_up(blk, 1, 64);
            if (lane == 0) prev = f0 > first ? (csr_idx[f0 - 1] - p_eff) >> 6 : -1;
            const bool start = blk >= 0 && blk != prev;
            const unsigned long long bal = __ballot(start);
            int at = 0;
            if (lane == 0 && bal) at = atomicAdd(&sh_count, (int)__popcll(bal));
            at = __shfl(at, 0, 64);
            if (start) {
                float m = csr_r[f];
                for (int32_t g = f + 1; g < end && ((csr_idx[g] - p_eff) >> 6) == blk; g++) m = fmaxf(m, csr_r[g]);
                y_pk[base + at + __popcll(bal & ((1ull << lane) - 1ull))] = (uint32_t)blk | ((uint32_t)__half_as_ushort(__float2half(m)) << 16);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) { co2[2 * k] = base; co2[2 * k + 1] = base + sh_count; }
        __syncthreads();     // sh_count is read before the next user resets it
    }
}
__global__ __launch_bounds__(256) void k_tail_blocks(const CsrDesc* __restrict__ D, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr_idx,
                                                     const float* __restrict__ csr_r, uint32_t* __restrict__ y_pk, int32_t* __restrict__ co_tail_all) {
    const CsrDesc d = D[blockIdx.y];
    if (!d.has_tail) return;       // block-uniform
    tail_blocks_body(d.slot_base, d.n_slots, d.p_eff, rowptr, csr_idx, csr_r, y_pk, co_tail_all + d.co_tail_off);
}

// ================================================================ chunk offsets for the row kernel
__device__ __forceinline__ void chunk_offsets_body(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr_idx, int32_t slot_base,
                                                   int32_t n_slots, int32_t CH, int32_t nch, int32_t* __restrict__ chunk_off) {
    const int64_t total = (int64_t)n_slots * (nch + 1);
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t v = (int32_t)(t / (nch + 1)), ch = (int32_t)(t % (nch + 1));
        const int32_t a = rowptr[slot_base + v], b = rowptr[slot_base + v + 1];
        int32_t lo = a, hi = b;
        const int32_t key = ch * CH;   // first entry with idx >= key
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (csr_idx[mid] < key) lo = mid + 1; else hi = mid;
        }
        chunk_off[t] = (ch == nch) ? b : lo;
    }
}
__global__ void k_chunk_offsets(const CsrDesc* __restrict__ D, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr_idx,
                                int32_t* __restrict__ co_all) {
    const CsrDesc d = D[blockIdx.y];
    chunk_offsets_body(rowptr, csr_idx, d.slot_base, d.n_slots, d.CH, d.nch, co_all + d.co_off);
}

// ---- segment tables (fy_cooc.hpp; SegDesc: fy_rm2_tables.hpp): counts, exclusive prefix, fill.  A table's counts / prefixes are a
// range of one array (cnt_off), so ONE scan numbers the segments of all tables and one fill writes them -- built cluster by
// cluster the same 25 M CSC entries cost ~15 small launches and a host round trip per cluster: 20 ms at 50 clusters against 4.6 ms
// for the one-cluster job.

#ifndef FY_SAMPLE_SHIFT
#define FY_SAMPLE_SHIFT 6     // the symmetric cut searches every 64th CSR entry (measured, ML-25M job, tables / row kernel ms: exact cut 4.57 / 7.84; stride 64: 2.96 / 8.48 = 25.6 ms per job; stride 16: 3.23 / 8.21 = 25.7; Netflix shape 77.1 / 79.1 ms per job)
#endif
__device__ __forceinline__ void seg_counts_body(const SegDesc& d, const SegArrays& A, int32_t* __restrict__ cnt, int32_t* __restrict__ start_all) {
    const int32_t* __restrict__ csc_slot = A.csc_slot;
    const int32_t* __restrict__ chunk_off = A.chunk_off + d.co_off;
    const int32_t* __restrict__ row_of_entry = A.row_of_entry;      // [q0 + q]: the row (rank inside the cluster) of CSC entry q
    const int32_t slot_base = d.slot_base, q0 = d.q0, nq = d.nq, nch = d.nch;
    const bool rows = d.half || d.lim_chunks > 0;
    // one thread per CSC entry: the rater's nch + 1 chunk offsets are one contiguous gather -- ONE 16-byte load where a row of the
    // table is four offsets (three chunks: ML-25M shape).  Round 4: the kernel ran at 72 % of the L2's request rate (6.5 requests per
    // entry, TCP_TCC_READ_REQ), most of them the same 16 bytes fetched offset by offset from 64 different rows per wave instruction.
    const bool row4 = nch == 3 && (reinterpret_cast<uintptr_t>(chunk_off) & 15) == 0;      // (kernel-uniform)
    const bool row2 = nch == 1 && (reinterpret_cast<uintptr_t>(chunk_off) & 7) == 0;       // one chunk (Netflix shape): two offsets, 8 bytes
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q <= nq; q += (int64_t)gridDim.x * blockDim.x) {
        const bool live = q < nq && !(d.only_from > 0 && row_of_entry[q0 + q] < d.only_from);
        const int32_t* co = live ? chunk_off + (int64_t)(csc_slot[q0 + q] - slot_base) * (nch + 1) : nullptr;
        int4 c4 = make_int4(0, 0, 0, 0);
        if (live && row4) c4 = *reinterpret_cast<const int4*>(co);
        if (live && row2) { const int2 v = *reinterpret_cast<const int2*>(co); c4.x = v.x; c4.y = v.y; }
        auto CO = [&](int k) -> int32_t { return (row4 || row2) ? (k == 0 ? c4.x : k == 1 ? c4.y : k == 2 ? c4.z : c4.w) : co[k]; };
        int32_t prev = live ? CO(0) : 0;
        int32_t own = -1, behind = 0, climit = nch;
        const int32_t r_e = (live && rows) ? row_of_entry[q0 + q] : 0;
        if (live && d.lim_chunks > 0 && r_e >= d.lim_from) climit = d.lim_chunks;
        if (live && d.half && (d.sym_rows == 0 || r_e < d.sym_rows)) {
            const int32_t r = r_e;
            own = r / d.CH;
            // Where does the slice behind (v, i) start?  Exactly: behind the position of i in the rater's row -- a binary search over the
            // row slice in the 100-400 MB csr_idx per CSC entry (1.6 ms of the ML-25M job, 10.6 ms at Netflix shape, round 2).  Now: the
            // last aligned CSR position inside the slice whose entry is <= r, found in the SAMPLES (every 2^FY_SAMPLE_SHIFT-th entry: a few MB,
            // cache-resident, a handful of probes); the few entries between it and i are masked by the row kernel (column <= row).
            constexpr int SS = FY_SAMPLE_SHIFT;
            const int32_t co_own = CO(own), co_next = CO(own + 1);
            int32_t klo = (co_own + (1 << SS) - 1) >> SS, khi = (co_next + (1 << SS) - 1) >> SS;      // samples inside the slice: [klo, khi)
            while (klo < khi) {                                                    // first k with samp[k] > r
                const int32_t mid = (klo + khi) >> 1;
                if (A.samples[mid] <= r) klo = mid + 1; else khi = mid;
            }
            const int32_t lo = max(co_own, (klo - 1) << SS);                      // (no sample <= r inside the slice: its beginning)
            behind = lo;
            start_all[q0 + q] = lo;
        }
        for (int32_t ch = 0; ch < nch; ch++) {
            int32_t n = 0;
            if (live) {
                const int32_t next = CO(ch + 1);
                const int32_t first = ch == own ? behind : prev;
                n = ((d.rect ? (own >= 0 && ch > own) : ch < own) || ch >= climit) ? 0 : (next - first + 63) >> 6;
                prev = next;
            }
            cnt[(int64_t)ch * (nq + 1) + q] = n;
        }
    }
}
__global__ void k_seg_counts(const SegDesc* __restrict__ D, SegArrays A, int32_t* __restrict__ cnt_all, int32_t* __restrict__ start_all) {
    const SegDesc d = D[blockIdx.y];
    seg_counts_body(d, A, cnt_all + d.cnt_off, start_all);
}

// One wave fills the segments of 64 consecutive CSC entries of one chunk cooperatively: the group's segments are
// contiguous in the table (exclusive prefix `ptr`), lane l writes segment base + l, base + l + 64, ... after finding its
// owner among the 64 entries with a binary search over shuffled prefix values -- every store of the 3 GB table is
// coalesced (one thread per entry writing its own run of segments reached 1.1 TB/s).
__device__ __forceinline__ void seg_fill_body(const SegDesc& d, const SegArrays& A, const int32_t* __restrict__ ptr, const int32_t* __restrict__ start_all,
                                              int2* __restrict__ seg, float* __restrict__ seg_w) {
    const int32_t* __restrict__ csc_slot = A.csc_slot;
    const float* __restrict__ csc_w = A.csc_w;
    const int32_t* __restrict__ chunk_off = A.chunk_off + d.co_off;
    const int32_t* __restrict__ row_of_entry = A.row_of_entry;
    const int32_t slot_base = d.slot_base, q0 = d.q0, nq = d.nq, nch = d.nch;
    // A wave takes the group's entries through up to CB chunks at once: what is per ENTRY (rater slot, row, weight) is loaded once, and the
    // loads that are per (entry, chunk) -- chunk offsets, segment prefixes -- are all in flight before the first segment is written.
    // (Round 4: one (group, chunk) per wave iteration meant one dependent chain slot -> chunk offsets -> prefix per ~100 segments: the fill
    // ran at 1.4 TB/s of stores, bound by that latency.)
    constexpr int CB = 4;
    const bool row4 = nch == 3 && (reinterpret_cast<uintptr_t>(chunk_off) & 15) == 0;      // a table row = four offsets = one 16-byte load
    const bool row2 = nch == 1 && (reinterpret_cast<uintptr_t>(chunk_off) & 7) == 0;       // two offsets = one 8-byte load
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    const int64_t n_groups = ((int64_t)nq + 63) >> 6;
    const int32_t n_cb = (nch + CB - 1) / CB;
    const int64_t total_work = n_groups * n_cb;
    for (int64_t gw = blockIdx.x * (int64_t)wpb + (threadIdx.x >> 6); gw < total_work; gw += (int64_t)gridDim.x * wpb) {
        const int32_t ch0 = (int32_t)(gw / n_groups) * CB;
        const int64_t g = gw - (int64_t)(ch0 / CB) * n_groups;
        const int64_t q = g * 64 + lane;
        const int64_t q_end = min((int64_t)nq, g * 64 + 64);
        const bool live = q < nq;
        int32_t cov[CB + 1], startv[CB], endv[CB];
        int32_t r = 0, own = -1, own_start = 0;
        bool dead = false, limited = false;
        float w = 0.0f;
#pragma unroll
        for (int c = 0; c < CB; c++) {      // (wave-uniform tests)
            startv[c] = 0;
            endv[c] = ch0 + c < nch ? ptr[(int64_t)(ch0 + c) * (nq + 1) + q_end] : 0;
            if (live && ch0 + c < nch) startv[c] = ptr[(int64_t)(ch0 + c) * (nq + 1) + q];
        }
#pragma unroll
        for (int c = 0; c <= CB; c++) cov[c] = 0;
        if (live) {
            const int32_t* co = chunk_off + (int64_t)(csc_slot[q0 + q] - slot_base) * (nch + 1) + ch0;
            if (row4) {
                const int4 v = *reinterpret_cast<const int4*>(co);      // (ch0 = 0: the whole row)
                cov[0] = v.x; cov[1] = v.y; cov[2] = v.z; cov[3] = v.w;
            } else if (row2) {
                const int2 v = *reinterpret_cast<const int2*>(co);
                cov[0] = v.x; cov[1] = v.y;
            } else {
#pragma unroll
                for (int c = 0; c <= CB; c++)
                    if (ch0 + c <= nch) cov[c] = co[c];
            }
            if (d.half || d.lim_chunks > 0) {
                r = row_of_entry[q0 + q];
                if (d.half && (d.sym_rows == 0 || r < d.sym_rows)) {
                    own = r / d.CH;
                    if (own >= ch0 && own < ch0 + CB) own_start = start_all[q0 + q];
                }
                limited = d.lim_chunks > 0 && r >= d.lim_from;
            }
            if (d.only_from > 0 && row_of_entry[q0 + q] < d.only_from) dead = true;
            w = csc_w[q0 + q];
        }
#pragma unroll
        for (int c = 0; c < CB; c++) {
            const int32_t ch = ch0 + c;
            if (ch >= nch) break;                             // wave-uniform
            int32_t f0 = cov[c], len = cov[c + 1] - cov[c], start = startv[c];
            if (live) {
                if (own >= 0) {
                    if (d.rect ? ch > own : ch < own) len = 0;
                    else if (ch == own) { f0 = own_start; len = cov[c + 1] - f0; }
                }
                if (limited && ch >= d.lim_chunks) len = 0;
                if (dead) len = 0;
            } else len = 0;
            const int32_t base = __shfl(start, 0, 64);
            const int32_t total = endv[c] - base;                 // segments of the whole group
            if (!live) start = base + total;                      // inactive lanes sit behind the last segment
            const int32_t rel = start - base;
            for (int32_t kk = 0; kk < total; kk += 64) {         // wave-uniform trip count: the shuffles need every lane alive
                const int32_t k = kk + lane;
                int lo = 0, hi = 63;                              // largest lane j with rel_j <= k (rel is non-decreasing)
#pragma unroll
                for (int it = 0; it < 6; it++) {
                    const int mid = (lo + hi + 1) >> 1;
                    const int32_t rm = __shfl(rel, mid, 64);
                    if (rm <= k) lo = mid; else hi = mid - 1;
                }
                // entries with zero segments share their rel with the next entry: the owner is the LAST lane with rel <= k
                const int32_t off = k - __shfl(rel, lo, 64);
                const int32_t of0 = __shfl(f0, lo, 64), olen = __shfl(len, lo, 64);
                const float ow = __shfl(w, lo, 64);
                if (k < total) {
                    seg[base + k] = make_int2(of0 + 64 * off, min(64, olen - 64 * off));
                    seg_w[base + k] = ow;
                }
            }
        }
    }
}
__global__ void k_seg_fill(const SegDesc* __restrict__ D, SegArrays A, const int32_t* __restrict__ ptr_all, const int32_t* __restrict__ start_all,
                           int2* __restrict__ seg, float* __restrict__ seg_w) {
    const SegDesc d = D[blockIdx.y];
    seg_fill_body(d, A, ptr_all + d.cnt_off, start_all, seg, seg_w);
}

__global__ void k_csr_samples(int64_t n_samples, const int32_t* __restrict__ csr_idx, int32_t* __restrict__ samp) {
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n_samples; k += (int64_t)gridDim.x * blockDim.x) samp[k] = csr_idx[k << FY_SAMPLE_SHIFT];
}
// every 64th entry of csr_idx (what the symmetric cut of the segment tables searches, SegArrays::samples)
void build_csr_samples(Context* ctx, int64_t nnz, const int32_t* csr_idx, DevBuf<int32_t>& samp, hipStream_t st) {
    const int64_t n = (nnz + (1 << FY_SAMPLE_SHIFT) - 1) >> FY_SAMPLE_SHIFT;
    samp.alloc(ctx, (size_t)n + 1);
    if (n) k_csr_samples<<<grid_for(n), 256, 0, st ? st : ctx->stream>>>(n, csr_idx, samp.get());
    FY_KERNEL_CHECK();
}

// ---- host side.  Launch shapes: one table keeps the grid caps of the one-table build it replaces, several tables (grid.y) those of the
// all-clusters build.
static dim3 table_grid(int64_t threads, size_t n_tables, int cap_one, int cap_many) {
    return dim3((unsigned)grid_for(threads, 256, n_tables == 1 ? cap_one : cap_many), (unsigned)n_tables);
}
// Descriptors go to the device as kernel ARGUMENTS, 2 KB per launch: a launch is queued like the kernels that read them, where a
// pageable hipMemcpyAsync of 64 bytes stages, blits and costs the one-table build ~20 us each (measured: tables of the one-cluster
// job + 0.03 ms with two such copies, profiles/cooc_tables).
template <class T>
struct DescPack {
    T d[2048 / sizeof(T)];
};
template <class T>
__global__ void k_put_descs(DescPack<T> p, int n, T* __restrict__ out) {
    if ((int)threadIdx.x < n) out[threadIdx.x] = p.d[threadIdx.x];
}
template <class T>
static void upload_descs(const std::vector<T>& h, T* d, hipStream_t st) {
    constexpr size_t cap = sizeof(DescPack<T>) / sizeof(T);
    static_assert(cap <= 64, "one thread per descriptor");
    for (size_t first = 0; first < h.size(); first += cap) {
        DescPack<T> p;
        const size_t n = std::min(cap, h.size() - first);
        std::copy(h.begin() + first, h.begin() + first + n, p.d);
        k_put_descs<T><<<1, 64, 0, st>>>(p, (int)n, d + first);
        FY_KERNEL_CHECK();
    }
}
CsrDescs upload_csr_descs(Context* ctx, std::vector<CsrDesc> h, hipStream_t st) {
    CsrDescs C{std::move(h), DevBuf<CsrDesc>()};
    C.d.alloc(ctx, C.h.size());
    upload_descs(C.h, C.d.get(), st ? st : ctx->stream);
    return C;
}
void build_chunk_offsets(Context* ctx, const CsrDescs& C, const int32_t* rowptr, const int32_t* csr_idx, int32_t* co_all, hipStream_t st) {
    int64_t most = 0;
    for (auto& d : C.h) most = std::max(most, (int64_t)d.n_slots * (d.nch + 1));
    if (most == 0) return;
    k_chunk_offsets<<<table_grid(most, C.h.size(), 4096, 1024), 256, 0, st ? st : ctx->stream>>>(C.d.get(), rowptr, csr_idx, co_all);
    FY_KERNEL_CHECK();
}
void pack_csr(Context* ctx, const CsrDescs& C, const int32_t* csr_idx, const float* csr_r, uint32_t* pk, hipStream_t st) {
    int64_t most = 0;
    for (auto& d : C.h) most = std::max<int64_t>(most, d.f1 - d.f0);
    if (most == 0) return;
    k_pack_csr<<<table_grid(most, C.h.size(), 4096, 1024), 256, 0, st ? st : ctx->stream>>>(C.d.get(), csr_idx, csr_r, pk);
    FY_KERNEL_CHECK();
}

// The segment tables of all groups: counts, ONE scan, ONE read-back of the total, fill, and the closing synchronisation, after
// which the counts, the cut starts and the descriptors go back to the allocator (and the caller may release the groups' arrays).
void build_segment_tables(Context* ctx, const SegGroup* groups, size_t n_groups, SegStore& out, hipStream_t st) {
    if (!st) st = ctx->stream;
    std::vector<SegDesc> h;
    int64_t cnt_total = 0, n_start = 0;
    for (size_t g = 0; g < n_groups; g++)
        for (size_t k = 0; k < groups[g].n; k++) {
            const SegDesc& d = groups[g].desc[k];
            if (d.half && !groups[g].in.samples) FY_FAIL(FY_ERR_STATE, "internal: the symmetric segment table needs the CSR samples");
            h.push_back(d);
            cnt_total = std::max(cnt_total, d.cnt_off + seg_desc_counts(d));
            if (d.half) n_start = std::max(n_start, (int64_t)d.q0 + d.nq);
        }
    out.n_seg = 0;
    if (h.empty()) return;
    DevBuf<SegDesc> dd(ctx, h.size());
    DevBuf<int32_t> cnt(ctx, (size_t)cnt_total), start(ctx, (size_t)n_start + 1);
    out.ptr.alloc(ctx, (size_t)cnt_total);
    upload_descs(h, dd.get(), st);
    auto for_groups = [&](auto launch) {
        size_t first = 0;
        for (size_t g = 0; g < n_groups; first += groups[g].n, g++) {
            int32_t max_nq = 0, max_nch = 1;
            for (size_t k = 0; k < groups[g].n; k++) { max_nq = std::max(max_nq, groups[g].desc[k].nq); max_nch = std::max(max_nch, groups[g].desc[k].nch); }
            if (groups[g].n) launch(groups[g], dd.get() + first, max_nq, max_nch);
        }
    };
    for_groups([&](const SegGroup& G, const SegDesc* D, int32_t max_nq, int32_t) {
        k_seg_counts<<<table_grid((int64_t)max_nq + 1, G.n, 4096, 2048), 256, 0, st>>>(D, G.in, cnt.get(), start.get());
        FY_KERNEL_CHECK();
    });
    exclusive_scan_i32(ctx, cnt.get(), out.ptr.get(), (size_t)cnt_total, st);
    int32_t total = 0;   // the last count of every table is 0 by construction: the last prefix is the total
    FY_HIP(hipMemcpyAsync(&total, out.ptr.get() + (cnt_total - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FY_HIP(hipStreamSynchronize(st));       // the ONE host round trip of the tables
    out.n_seg = total;
    out.seg.alloc(ctx, (size_t)std::max(1, total));
    out.w.alloc(ctx, (size_t)std::max(1, total));
    for_groups([&](const SegGroup& G, const SegDesc* D, int32_t max_nq, int32_t max_nch) {
        if (max_nq == 0) return;
        const int64_t waves = (((int64_t)max_nq + 63) >> 6) * (G.n == 1 ? max_nch : (max_nch > 1 ? 4 : 1));
        k_seg_fill<<<table_grid(waves * 64, G.n, 256 * 64, 4096), 256, 0, st>>>(D, G.in, out.ptr.get(), start.get(), out.seg.get(), out.w.get());
        FY_KERNEL_CHECK();
    });
    FY_HIP(hipStreamSynchronize(st));
}
