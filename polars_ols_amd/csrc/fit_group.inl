// fit_group.inl -- the pieces of the one-wave-per-group kernels (64 threads: solve, resid, finish) of K14 (k14_iv.hip), K16
// (k16_absorb.hip), K17 (k17_absorb2.hip) and K18 (k18_glsar.hip): the item range of a group, the sum of its items' partials into LDS,
// A^-1 through the inverse of a Cholesky factor, the coefficient store in the batch's dtype, the se / t / p stores and the se / t / p of
// the absorb pair.  The factorisation and the solve are fit_solve.inl's; the LDS layouts of the solve kernels are in fit_lds.hpp.
#pragma once
#include "fit_solve.inl"
#include "k7_stats.hpp"

namespace pols {

// the items [v0, v1) of group g: its segments (ensure_segments) or the group itself.  Args: seg_offs, seg_first.
template <typename Args>
__device__ __forceinline__ void fit_group_items(const Args &a, const int64_t g, int64_t &v0, int64_t &v1) {
    v0 = a.seg_offs ? a.seg_first[g] : g;
    v1 = a.seg_offs ? a.seg_first[g + 1] : g + 1;
}

// dst[en] (LDS), en < count: element en of the partials (`stride` doubles per item) summed over the items [v0, v1) one after the other,
// in item order.  Returns whether every sum is finite, the same in every lane.  All 64 lanes of one wave call it; the caller puts a
// fit_wave_sync() behind it before another lane's sums are read.
__device__ __forceinline__ bool fit_sum_parts(const double *part, const size_t stride, const int64_t v0, const int64_t v1, const int count,
                                              double *dst, const int lane) {
    bool fin = true;
    for (int en = lane; en < count; en += 64) {
        double v = 0.0;
        for (int64_t it = v0; it < v1; ++it) v += part[(size_t)it * stride + en];
        dst[en] = v;
        fin = fin && fabs(v) <= FIT_DBL_MAX;
    }
    return __ballot(!fin) == 0;
}

// A: the factor fit_chol_factor left (k x (k + 1), lower triangle).  Lane c < k substitutes column c of its inverse into Ri (k x k, LDS);
// behind a fit_wave_sync() the k x k entries of A^-1 = Ri'Ri are spread over the lanes and go to inv (LDS or global).
__device__ __forceinline__ void fit_chol_inverse(const double *A, double *Ri, double *inv, const int k, const int lane) {
    const int LD = k + 1;
    if (lane < k) {
        for (int j = 0; j < k; ++j) {
            double s = j == lane ? 1.0 : 0.0;
            for (int i = lane; i < j; ++i) s = fma(-A[j * LD + i], Ri[i * k + lane], s);
            Ri[j * k + lane] = j < lane ? 0.0 : s / A[j * LD + j];
        }
    }
    fit_wave_sync();
    for (int p = lane; p < k * k; p += 64) {
        const int i = p / k, j = p - i * k;
        double v = 0.0;
        for (int l = i > j ? i : j; l < k; ++l) v = fma(Ri[l * k + i], Ri[l * k + j], v);
        inv[p] = v;
    }
}

// coefficient j of group g (kc per group) in the batch's dtype, when coef is wanted.  Args: coef, f32.
template <typename Args>
__device__ __forceinline__ void fit_store_coef(const Args &a, const int64_t g, const int kc, const int j, const double v) {
    if (!a.coef) return;
    if (a.f32) static_cast<float *>(a.coef)[(size_t)g * kc + j] = (float)v;
    else static_cast<double *>(a.coef)[(size_t)g * kc + j] = v;
}

// se / t / p of coefficient j of group g, each when it is wanted (a group without a fit: NaN).  Args: se, t_values, p_values.
template <typename Args>
__device__ __forceinline__ void fit_store_stats(const Args &a, const int64_t g, const int kc, const int j, const double se, const double tv,
                                                const double pv) {
    if (a.se) a.se[(size_t)g * kc + j] = se;
    if (a.t_values) a.t_values[(size_t)g * kc + j] = tv;
    if (a.p_values) a.p_values[(size_t)g * kc + j] = pv;
}

// se / t / p of one coefficient b from its variance v (NaN stays NaN, a negative variance too); dfp: the degrees of freedom of the t
__device__ __forceinline__ void fit_se_t_p(const double v, const double b, const double dfp, double &se, double &tv, double &pv) {
    if (v >= 0.0) {
        se = sqrt(v);
        tv = b / se;
        pv = (tv != tv) ? fit_nan() : k7_betai(0.5 * dfp, 0.5, dfp / (dfp + tv * tv));
    }
}

}  // namespace pols
