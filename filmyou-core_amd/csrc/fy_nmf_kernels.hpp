// fy_nmf_kernels.hpp -- what the factorisation (fy_nmf.hip) and the fold-in of given profiles (fy_foldin.hip) share, so that a
// row folded in on fixed factors carries the bits the factorisation's own H update would give it: the limits, the row body of
// the multiplicative update, and the Gram matrix launcher.
#pragma once
#include <cfloat>

#include "fy_common.hpp"

namespace fy {

constexpr int NMF_MAX_K = 256;
constexpr int NMF_GRAM_BLOCKS = 256;
constexpr int NMF_CHUNK = 512;      // entries of a row one wave sums sequentially (k_nmf_spmm_chunks)

__device__ __forceinline__ double fy_clampinf(double v) { return isinf(v) ? (v > 0 ? DBL_MAX : -DBL_MAX) : v; }

// One row of the multiplicative update, by one wave (lanes over the k columns, c = lane + 64 q):
//     res_c = m_c * x_c / (y_c + eps),  y = C m  (a ascending from 0.0).
// mode 0: HComputationReducer; 1: PPCHComputationReducer (d = m.y, e = m.x through the xor butterfly; + the optional L1
// normalisation); 2: WComputationMapper (infinities clamped).  m: the row (k doubles any lane may read: HBM, or a per-wave LDS row);
// x: the lane's columns of the SpMM row, 0.0 beyond k; C: k x k with leading dimension ldc.
__device__ __forceinline__ void nmf_update_row(int32_t k, int lane, const double* __restrict__ m, const double (&x)[NMF_MAX_K / 64],
                                               const double* __restrict__ C, int ldc, int mode, int normalize, double (&out)[NMF_MAX_K / 64]) {
    const double eps = 1e-12;   // MatrixComputationJob.java:41
    double y[NMF_MAX_K / 64], mv[NMF_MAX_K / 64];
    double d = 0.0, e = 0.0;
#pragma unroll
    for (int q = 0; q < NMF_MAX_K / 64; q++) {
        const int c = lane + 64 * q;
        y[q] = 0.0; mv[q] = 0.0;
        if (c < k) {
            double s = 0.0;
            for (int a = 0; a < k; a++) s += C[(int64_t)c * ldc + a] * m[a];
            y[q] = s;
            mv[q] = m[c];
            d += mv[q] * y[q];
            e += mv[q] * x[q];
        }
    }
    if (mode == 1) {
        for (int o = 32; o > 0; o >>= 1) { d += __shfl_xor(d, o, 64); e += __shfl_xor(e, o, 64); }
    }
    double res[NMF_MAX_K / 64], l1 = 0.0;
#pragma unroll
    for (int q = 0; q < NMF_MAX_K / 64; q++) {
        const int c = lane + 64 * q;
        res[q] = 0.0;
        if (c < k) {
            double xx = x[q], yy = y[q];
            if (mode == 1) { xx = fy_clampinf(xx + d); yy = fy_clampinf(yy + e); }
            else if (mode == 2) { xx = fy_clampinf(xx); yy = fy_clampinf(yy); }
            res[q] = mv[q] * (xx / (yy + eps));
            l1 += fabs(res[q]);
        }
    }
    if (normalize) {
        for (int o = 32; o > 0; o >>= 1) l1 += __shfl_xor(l1, o, 64);
    }
#pragma unroll
    for (int q = 0; q < NMF_MAX_K / 64; q++) out[q] = normalize ? res[q] / l1 : res[q];
}

// C = M^T M (M: n_rows x k in HBM) by k_nmf_gram_partial / k_nmf_gram_sum with NMF_GRAM_BLOCKS; part: NMF_GRAM_BLOCKS x k x k
void nmf_gram(Context* ctx, int32_t n_rows, int32_t k, const double* M, double* part, double* C);

}  // namespace fy
