// k7_stats.hpp -- K7 "group_statistics": the mode="statistics" side-car (src/statistics.rs) for every group.
#pragma once
#include "common.hpp"

namespace pols {

struct StatsArgs {
    const void *y;
    const void *w;
    const void *x[POLS_MAX_FEATURES];
    const int64_t *offs;
    int64_t n_groups;
    const double *gram;   // n_groups x NZ x NZ from gram_stream (Z = [sqrt(w) X | sqrt(w) 1 | sqrt(w) y])
    const void *coef;     // n_groups x kt dispatcher coefficients, batch dtype
    double lambda;        // kwargs.alpha (src/expressions.rs:474)
    double *r2, *mae, *mse, *se, *tv, *pv;
    int32_t *status;
    int32_t k_user, kt;
    // LONG groups cut into segments (api.hip: ensure_segments) or nullptr: the row passes run one workgroup per SEGMENT, their sums
    // meet per group in segment order (k7_stats_launch then runs prepare / segment sums / finish instead of the one kernel)
    const int64_t *seg_offs;   // n_seg + 1
    const int32_t *seg_map;    // segment -> group
    const int32_t *seg_first;  // group -> first segment, n_groups + 1
    int64_t n_seg;
    double *seg_part;          // n_seg x 5 partial sums
    double *prep;              // n_groups x (3 kt + 1): dispatcher coefficients, A^-1 X'y, diag(A^-1), factorisation ok
    double *rss;               // optional, n_groups: the side-car's residual sum of squares (what sigma^2 = rss / df divides); nullptr for
                               // every caller but the influence entry (K7i)
};

int k7_stats_launch(pols_ctx *ctx, int dtype, const StatsArgs &a);

constexpr int K7_KMAX = 31;   // columns (incl. the intercept) of the K7 kernels; wider statistics run on K8

#if defined(__HIPCC__)
// Two-sided Student-t p-value 2 (1 - cdf(|t|)) == I_{df/(df+t^2)}(df/2, 1/2): regularised incomplete beta by Lentz' continued
// fraction (what statrs 0.17.1 evaluates for src/statistics.rs:45-49).  Shared by K7 and the wide statistics kernel (K8).
__device__ inline double k7_betacf(double a, double b, double x) {
    const double tiny = 1e-300;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 500; ++m) {
        const int m2 = 2 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d; h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 1e-16) break;
    }
    return h;
}

// regularised incomplete beta I_x(a, b)
__device__ inline double k7_betai(double a, double b, double x) {
    if (!(x > 0.0)) return (x != x) ? x : 0.0;
    if (x >= 1.0) return 1.0;
    const double bt = exp(lgamma(a + b) - lgamma(a) - lgamma(b) + a * log(x) + b * log1p(-x));
    if (x < (a + 1.0) / (a + b + 2.0)) return bt * k7_betacf(a, b, x) / a;
    return 1.0 - bt * k7_betacf(b, a, 1.0 - x) / b;
}

// regularised upper incomplete gamma Q(a, x) = Gamma(a, x) / Gamma(a), the chi2(2a) upper tail at 2x: the series of P below
// x < a + 1, Lentz' continued fraction of Q above (K14's Sargan p-value)
__device__ inline double k7_gammaq(double a, double x) {
    if (!(x >= 0.0) || !(a > 0.0)) return __longlong_as_double(0x7ff8000000000000LL);
    if (x == 0.0) return 1.0;
    if (x > 1.79769313486231570815e308) return 0.0;
    const double ft = exp(a * log(x) - x - lgamma(a));
    if (x < a + 1.0) {
        double ap = a, del = 1.0 / a, sum = del;
        for (int m = 1; m <= 1000; ++m) {
            ap += 1.0;
            del *= x / ap;
            sum += del;
            if (fabs(del) < fabs(sum) * 1e-16) break;
        }
        return 1.0 - sum * ft;
    }
    const double tiny = 1e-300;
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int m = 1; m <= 1000; ++m) {
        const double an = -(double)m * ((double)m - a);
        b += 2.0;
        d = an * d + b; if (fabs(d) < tiny) d = tiny;
        c = b + an / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 1e-16) break;
    }
    return ft * h;
}

// wave 0 of the group: A = X'X + lambda I factored, A^-1 X'y and diag(A^-1) (src/statistics.rs:100-121), the dispatcher's coefficients.
// Shared by K7 and the robust covariance kernels (K7r), which keep all of M = L^-1 to form the whole A^-1 = M'M.
template <typename T>
__device__ __forceinline__ void k7_small_solve(const StatsArgs &a, int64_t g, int lane, double *L, double *M, double *rinv, double *bvec,
                                               double *tvec, double *binv, double *cdis, double *dg, int *okflag_p) {
    const int kt = a.kt, NZ = kt + 1;
    const double *G = a.gram + (size_t)g * NZ * NZ;
    int &okflag = *okflag_p;
    {
        for (int q = lane; q < kt * kt; q += 64) {
            const int i = q / kt, j = q - i * kt;
            L[q] = G[i * NZ + j] + (i == j ? a.lambda : 0.0);
        }
        if (lane < kt) {
            bvec[lane] = G[lane * NZ + kt];
            cdis[lane] = (double)static_cast<const T *>(a.coef)[g * kt + lane];
        }
        __builtin_amdgcn_wave_barrier();
        bool ok = true;
        for (int j = 0; j < kt; ++j) {
            double d = L[j * kt + j];
            for (int p = 0; p < j; ++p) d -= L[j * kt + p] * L[j * kt + p];
            ok = ok && (d > 0.0);                                   // also false for NaN
            const double ri = 1.0 / sqrt(d);
            if (lane == 0) rinv[j] = ri;
            if (lane > j && lane < kt) {
                double acc = L[lane * kt + j];
                for (int p = 0; p < j; ++p) acc -= L[lane * kt + p] * L[j * kt + p];
                L[lane * kt + j] = acc * ri;
            }
            __builtin_amdgcn_wave_barrier();
        }
        // M = L^-1, column c on lane c (forward substitution against e_c)
        if (lane < kt) {
            const int c = lane;
            for (int i = 0; i < c; ++i) M[i * kt + c] = 0.0;
            M[c * kt + c] = rinv[c];
            for (int i = c + 1; i < kt; ++i) {
                double acc = 0.0;
                for (int p = c; p < i; ++p) acc += L[i * kt + p] * M[p * kt + c];
                M[i * kt + c] = -acc * rinv[i];
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < kt) {
            double t = 0.0;
            for (int j = 0; j <= lane; ++j) t += M[lane * kt + j] * bvec[j];
            tvec[lane] = t;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < kt) {
            double bi = 0.0, dd = 0.0;
            for (int p = lane; p < kt; ++p) { const double m = M[p * kt + lane]; bi += m * tvec[p]; dd += m * m; }
            binv[lane] = bi;                                        // A^-1 X'y          (:116)
            dg[lane] = dd;                                          // diag(A^-1)
        }
        if (lane == 0) okflag = ok ? 1 : 0;
    }
}

#endif

}  // namespace pols
