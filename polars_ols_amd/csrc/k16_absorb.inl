// k16_absorb.inl -- the device pieces that K16 (k16_absorb.hip) and K17 (k17_absorb2.hip) share: the wave sum in the fixed DPP order, the
// column pointers in LDS, the group of a position, the one-wave solve behind the moments (Cholesky against the raw second moments, the
// two substitutions, A^-1) and the se / t / p stage of the finish launches.
#pragma once
#include "fit_solve.inl"
#include "k7_stats.hpp"

namespace pols {

// the sum over the wave in every lane, in the fixed order of the DPP steps; all 64 lanes active
__device__ __forceinline__ double k16_wave_sum(double v) { return readlane63(wave_sum_row3(v)); }

// the column pointers into LDS (a run-time index into the kernel arguments would put them in scratch).  Args: x, k_user.
template <typename Args>
__device__ __forceinline__ void k16_columns(const Args &a, const void **xp, const int tid) {
#pragma unroll
    for (int j = 0; j < POLS_MAX_FEATURES; ++j)
        if (tid == j && j < a.k_user) xp[j] = a.x[j];
}

// the group of position p: the last g with offs[g] <= p (the groups before it that start there are empty)
__device__ __forceinline__ int64_t k16_group_of(const int64_t *offs, int64_t n_groups, int64_t p) {
    int64_t lo = 0, hi = n_groups;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (offs[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// One wave.  Gs (LDS): the packed upper triangle of [X~ | y~]'[X~ | y~] (nz = k + 1); T: the k raw second moments the pivots are held
// against.  A (k x (k + 1)), d0 (k), rhs (k), Ri (k x k): LDS work.  `ok` in: the group has a fit to attempt (wave-uniform).  Returns
// whether b (in rhs) is usable; then A^-1 went to inv (k x k, global).
__device__ __forceinline__ bool k16_solve_core(bool ok, const double *Gs, const double *T, double *A, double *d0, double *rhs, double *Ri,
                                               double *inv, const int k, const int lane) {
    const int nz = k + 1, ne = nz * (nz + 1) / 2, LD = k + 1;
    if (ok) {
        for (int en = lane; en < ne; en += 64) {
            int i, j;
            tri_unpack(en, nz, i, j);
            const double v = Gs[en];
            if (j == k) { if (i < k) rhs[i] = v; }
            else { A[i * LD + j] = v; A[j * LD + i] = v; }
        }
        if (lane < k) d0[lane] = T[lane];                          // the pivots are held against the RAW second moments
        fit_wave_sync();
        ok = fit_chol_factor(A, d0, k, lane);
    }
    if (ok) {
        for (int j = 0; j < k; ++j) {                              // L z = g
            const double z = rhs[j] / A[j * LD + j];
            fit_wave_sync();
            if (lane == j) rhs[j] = z;
            else if (lane > j && lane < k) rhs[lane] -= A[lane * LD + j] * z;
            fit_wave_sync();
        }
        for (int j = k - 1; j >= 0; --j) {                         // L'b = z
            const double z = rhs[j] / A[j * LD + j];
            fit_wave_sync();
            if (lane == j) rhs[j] = z;
            else if (lane < j) rhs[lane] -= A[j * LD + lane] * z;
            fit_wave_sync();
        }
        const double v = lane < k ? rhs[lane] : 0.0;
        ok = __ballot(!(fabs(v) <= FIT_DBL_MAX)) == 0;
    }
    if (ok) {
        if (lane < k) {                                            // column `lane` of the inverse of the factor
            for (int j = 0; j < k; ++j) {
                double s = j == lane ? 1.0 : 0.0;
                for (int i = lane; i < j; ++i) s = fma(-A[j * LD + i], Ri[i * k + lane], s);
                Ri[j * k + lane] = j < lane ? 0.0 : s / A[j * LD + j];
            }
        }
        fit_wave_sync();
        for (int p = lane; p < k * k; p += 64) {                   // A^-1
            const int i = p / k, j = p - i * k;
            double v = 0.0;
            for (int l = i > j ? i : j; l < k; ++l) v = fma(Ri[l * k + i], Ri[l * k + j], v);
            inv[p] = v;
        }
    }
    return ok;
}

// se / t / p of one coefficient b from its variance v (NaN stays NaN, a negative variance too); dfp: the degrees of freedom of the t
__device__ __forceinline__ void k16_se_t_p(const double v, const double b, const double dfp, double &se, double &tv, double &pv) {
    if (v >= 0.0) {
        se = sqrt(v);
        tv = b / se;
        pv = (tv != tv) ? fit_nan() : k7_betai(0.5 * dfp, 0.5, dfp / (dfp + tv * tv));
    }
}

}  // namespace pols
