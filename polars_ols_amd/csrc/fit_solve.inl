// fit_solve.inl -- the one-wave Cholesky solve of K11 (k11_rlm.hip), K13 (k13_glm.hip), K14 (k14_iv.hip) and K18 (k18_glsar.hip): a
// packed Gram matrix in LDS goes to the coefficients by a right-looking factorisation (the trailing update spread over the lanes) and
// the two substitutions; K14 also takes the factorisation alone, and K16 / K17 (k16_solve_core, k16_absorb.inl) take it with pivots held
// against another diagonal.  What the one-wave-per-group kernels share around the solve is in fit_group.inl.
#pragma once
#include "fit_tile.inl"

namespace pols {

// LDS traffic between the lanes of ONE wave: its LDS operations complete in order, the compiler must not move them
__device__ __forceinline__ void fit_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A: a symmetric kt x kt matrix in LDS (row stride kt + 1), d0 its diagonal.  Right-looking factorisation in place: the factor L ends in
// the lower triangle of A.  A pivot fails when d^2 <= 16 kt eps A_jj; the result is false (in every lane) then.  All 64 lanes of one
// wave call it, behind a fit_wave_sync() after A and d0 were written.
__device__ __forceinline__ bool fit_chol_factor(double *A, const double *d0, const int kt, const int lane) {
    const int LD = kt + 1;
    bool ok = true;
    const double noise = 16.0 * (double)kt * FIT_EPS;
    for (int j = 0; j < kt; ++j) {
        const double d = A[j * LD + j];
        if (!(d > noise * d0[j])) { ok = false; break; }   // (wave-uniform: every lane read the same word)
        const double sd = sqrt(d);
        fit_wave_sync();
        if (lane >= j && lane < kt) A[lane * LD + j] = lane == j ? sd : A[lane * LD + j] / sd;
        fit_wave_sync();
        for (int p = lane; p < kt * kt; p += 64) {         // the trailing lower triangle: A[i][c] -= L[i][j] L[c][j], j < c <= i
            const int i = p / kt, c = p - i * kt;
            if (c > j && c <= i) A[i * LD + c] -= A[i * LD + j] * A[c * LD + j];
        }
        fit_wave_sync();
    }
    return ok;
}

// Gm: the packed upper triangle of the (kt + 1) x (kt + 1) matrix [A g; g' .] (row i holds the entries (i, i) .. (i, kt)).  Solves
// A b = g: b ends in rhs[0 .. kt), the factor L in the lower triangle of A (kt x (kt + 1), row-major), the diagonal of A in d0.  A pivot
// fails when d^2 <= 16 kt eps A_jj; the result is false (in every lane) then, and when a coefficient is not finite.  All 64 lanes of
// one wave call it; the caller puts a barrier behind it before other waves read the result.
__device__ __forceinline__ bool fit_chol_solve(const double *Gm, double *A, double *rhs, double *d0, const int kt, const int lane) {
    const int nz = kt + 1, ne = nz * (nz + 1) / 2, LD = kt + 1;
    for (int en = lane; en < ne; en += 64) {
        int i = 0, t = en;                                 // (tri_unpack, written out: through the call the compiler lays the blocks of
        while (t >= nz - i) { t -= nz - i; ++i; }          // this one-wave solve out differently, and the split GLM pair, which runs it
        const int j = i + t;                               // once per iteration on its critical path, measured 1.1 % slower)
        const double v = Gm[en];
        if (j == kt) { if (i < kt) rhs[i] = v; }
        else { A[i * LD + j] = v; A[j * LD + i] = v; if (i == j) d0[i] = v; }
    }
    fit_wave_sync();
    bool ok = fit_chol_factor(A, d0, kt, lane);
    if (ok) {
        for (int j = 0; j < kt; ++j) {                     // L z = g
            const double z = rhs[j] / A[j * LD + j];
            fit_wave_sync();
            if (lane == j) rhs[j] = z;
            else if (lane > j && lane < kt) rhs[lane] -= A[lane * LD + j] * z;
            fit_wave_sync();
        }
        for (int j = kt - 1; j >= 0; --j) {                // L'b = z
            const double z = rhs[j] / A[j * LD + j];
            fit_wave_sync();
            if (lane == j) rhs[j] = z;
            else if (lane < j) rhs[lane] -= A[j * LD + lane] * z;
            fit_wave_sync();
        }
        const double v = lane < kt ? rhs[lane] : 0.0;
        ok = __ballot(!(fabs(v) <= FIT_DBL_MAX)) == 0;   // every coefficient finite
    }
    return ok;
}

}  // namespace pols
