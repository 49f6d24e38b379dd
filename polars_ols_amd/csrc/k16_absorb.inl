// k16_absorb.inl -- the device pieces that K16 (k16_absorb.hip) and K17 (k17_absorb2.hip) share: the wave sum in the fixed DPP order, the
// column pointers in LDS, the group of a position, the one-wave solve behind the moments (Cholesky against the raw second moments, the
// two substitutions, A^-1), the head and the tail of the resid launches and the finish launch.  What every one-wave kernel of the fit
// entries shares is in fit_group.inl.
#pragma once
#include "fit_group.inl"
#include "fit_lds.hpp"

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

// One wave.  dyn: the kernel's LDS, cut by o (fit_lds.hpp).  Gs holds the packed upper triangle of [X~ | y~]'[X~ | y~] (nz = k + 1), T
// the k raw second moments the pivots are held against; A, d0, rhs, Ri are work.  `ok` in: the group has a fit to attempt
// (wave-uniform).  Returns whether b (in rhs) is usable; then A^-1 went to inv (k x k, global).  The two substitutions are a copy of
// fit_chol_solve's, which stays textually as it is (its comment: a neutral-looking change cost K13's split pair 1.1 %); folding the
// two into one is a follow-up.
__device__ __forceinline__ bool k16_solve_core(bool ok, double *dyn, const AbsorbLds &o, double *inv, const int k, const int lane) {
    const int nz = k + 1, ne = nz * (nz + 1) / 2, LD = k + 1;
    const double *Gs = dyn + o.Gs, *T = dyn + o.T;
    double *A = dyn + o.A, *d0 = dyn + o.d0, *rhs = dyn + o.rhs, *Ri = dyn + o.Ri;
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
    if (ok) fit_chol_inverse(A, Ri, inv, k, lane);
    return ok;
}

// The head of the resid launches (one wave per category).  st: the state row of the category's group (b at ob, A^-1 at oi); out: the
// category's partials.  A group without a fit (wave-uniform) gets zeros -- the finish writes NaN -- and false comes back: the wave
// returns.  Else b goes to bs and, with `cluster`, A^-1 to Ai (LDS; the caller's barrier publishes them).
__device__ __forceinline__ bool absorb_resid_head(const double *st, const int ob, const int oi, double *out, const bool cluster, const int k,
                                                  const int lane, double *bs, double *Ai) {
    if (st[1] == 0.0) {
        if (lane == 0) out[0] = 0.0;
        if (cluster && lane < k) out[1 + lane] = 0.0;
        return false;
    }
    if (lane < k) bs[lane] = st[ob + lane];
    if (cluster)
        for (int q = lane; q < k * k; q += 64) Ai[q] = st[oi + q];
    return true;
}

// ... and their tail: the wave sum of the lanes' rss, and with `cluster` z = A^-1 s_c (sacc, lane j < k: s_cj; ss: k doubles of LDS), its squares
__device__ __forceinline__ void absorb_resid_tail(const double rss, const double sacc, double *ss, const double *Ai, double *out,
                                                  const bool cluster, const int k, const int lane) {
    const double tot = k16_wave_sum(rss);
    if (lane == 0) out[0] = tot;
    if (cluster) {
        if (lane < k) ss[lane] = sacc;
        __syncthreads();
        if (lane < k) {
            double z = 0.0;
            for (int q = 0; q < k; ++q) z = fma(Ai[lane * k + q], ss[q], z);
            out[1 + lane] = z * z;
        }
    }
}

// The finish launch, one wave per group g.  st: the group's state row ([0] n, [1] fitted, [3] df, [5] y~'y~, [6] TSS, b at ob, A^-1 at
// oi); [c0i, c1i): the categories whose resid partials (stride rs: RSS_c, with cluster the k squares z_cj^2) are summed, lane l taking
// c0i + l, c0i + l + 64, ..; C: the clusters; d1: the denominator of the cluster correction (n - 1) / d1.
// Args: k_user, icpt, cluster, resid_part, se, t_values, p_values, sigma2, r2_within, r2.
template <typename Args>
__device__ __forceinline__ void absorb_finish(const Args &a, const int64_t g, const double *st, const int64_t c0i, const int64_t c1i,
                                              const size_t rs, const double C, const double d1, const int ob, const int oi) {
    const int lane = threadIdx.x, k = a.k_user, kc = k + a.icpt;
    const double n = st[0], df = st[3];
    const bool ok = st[1] != 0.0;                                  // (wave-uniform)
    const double q = fit_nan();
    double se = q, tv = q, pv = q, sigma2 = q, r2w = q, r2 = q;
    if (ok) {
        double l = 0.0;
        for (int64_t c = c0i + lane; c < c1i; c += 64) l += a.resid_part[(size_t)c * rs];
        const double rss = k16_wave_sum(l);
        sigma2 = rss / df;
        r2w = 1.0 - rss / st[5];
        r2 = 1.0 - rss / st[6];
        double v = q, dfp = df;
        if (a.cluster != 0) {
            double mine = 0.0;
            for (int j = 0; j < k; ++j) {
                double lz = 0.0;
                for (int64_t c = c0i + lane; c < c1i; c += 64) lz += a.resid_part[(size_t)c * rs + 1 + j];
                const double t = k16_wave_sum(lz);
                if (lane == j) mine = t;
            }
            dfp = C - 1.0;
            if (C >= 2.0 && d1 > 0.0) v = C / (C - 1.0) * (n - 1.0) / d1 * mine;
        } else if (lane < k) {
            v = sigma2 * st[oi + lane * k + lane];
        }
        if (lane < k) fit_se_t_p(v, st[ob + lane], dfp, se, tv, pv);
    }
    if (lane < kc) fit_store_stats(a, g, kc, lane, se, tv, pv);   // (the intercept's entries stay NaN)
    if (lane == 0) {
        if (a.sigma2) a.sigma2[g] = sigma2;
        if (a.r2_within) a.r2_within[g] = r2w;
        if (a.r2) a.r2[g] = r2;
    }
}

}  // namespace pols
