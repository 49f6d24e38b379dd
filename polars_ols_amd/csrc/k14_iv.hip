// k14_iv.hip -- K14: two-stage least squares (instrumental variables) per group with diagnostics (pols_iv2sls).
//
// Per group g, on the rows F_g that pols_least_squares fits with the excluded instruments counted as features (null policy, sqrt(w)
// scaling with a null weight acting as 1e-24), n = |F_g|: X = [X1 | X2 | 1] (kx columns, the n_endog columns X2 endogenous),
// Z = [X1 | 1 | Z2] (L = kx - n_endog + m columns), T = kx + m staged columns.
//   A = Z~'Z~ = R R',  Q = R^-1 Z~'X~,  r = R^-1 Z~'y~,  M = Q'Q (= X^'X^),  M b = Q'r,  Pi = R^-T Q (x^_i = Pi'z~_i),
//   e~_i = y~_i - x~_i'b (the ACTUAL regressors),  RSS = sum e~_i^2 (summed over rows),
//   V = sigma2 M^-1  |  M^-1 (sum e~_i^2 x^_i x^_i') M^-1 (HC0)  |  that x n / df (HC1),
//   first stage of endogenous column j, q its column of Q: RSS_u = x~'x~ - q'q, D = sum of q_l^2 over the rows of Z2 (Z2 is last in the
//   factorisation, so D is the drop in RSS from adding the excluded instruments), F = (D / m) / (RSS_u / (n - L)), D / (D + RSS_u),
//   Sargan S = n |r - Q b|^2 / RSS with the chi2(m - n_endog) upper tail.
// Everything is f64 on the inputs' values, for f32 batches too.  No atomics, every sum in a fixed order: two runs are bit-identical.
//
// Launches (one workgroup per segment of a long group -- ensure_segments -- or per group, unless said otherwise):
//   moments  K10's Gram launch (k10_gram_launch) over the concatenated column list [X1 | X2 | Z2 | 1 | y]: the packed upper triangle
//            of the (T + 1) x (T + 1) cross-moments and the fitted-row count per item.
//   solve    one wave per group: the partials summed in segment order, A and [C | Z~'y~] gathered from the moments, A factored
//            (fit_chol_factor), lane c substitutes column c of [Q | r], M and Q'r spread over the lanes, M b = Q'r by fit_chol_solve,
//            then the Sargan numerator, the first-stage diagnostics (lane j = endogenous column j), the inverse of M's factor (lane c =
//            column c), M^-1 and Pi.  b, M^-1 and Pi go to the group's state; coef, status, n_obs, first_stage_f and partial_r2 are final.
//            Dynamic LDS, sized by T: k14_solve_lds -- 39 440 bytes at kx = 30, L = 31 (T = 31); 2 632 at 3 + 2 + 1 regressors, 4 instruments.
//   rows     256-row tiles staged by fit_stage (16-byte streaming loads); the thread of a row computes e~_i and adds e~_i^2 to its own
//            sum, tiles in order; at the end DPP within a wave, the waves as (0 + 1) + (2 + 3).  ROBUST (HC0 / HC1): the thread also
//            forms x^_i = Pi'z~_i with Pi and b read at one LDS address by every lane (broadcasts), parks u_i = e~_i x^_i beside the
//            tile, and the kx (kx + 1) / 2 entries of sum u_i u_i' are accumulated with K10's entry-to-thread assignment (tri_spread).
//            Not launched when no wanted output needs a residual (coefficients and first-stage diagnostics: the frame is read once).
//            The plain form is given the regressors and y alone (a.k_user = n_feat, a.kt = kx) unless a null instrument drops rows.
//   finish   one wave per group: the items' partials summed in order, sigma2, V, se / t / p, Sargan and its p-value, cov.
//   predict  K10's prediction launch from the f64 coefficients (api.hip).
#include "k14_iv.hpp"
#include "k10_ridge_path.hpp"
#include "fit_launch.hpp"
#include "fit_group.inl"
#include "fit_lds.hpp"

namespace pols {

size_t k14_solve_lds(int kx, int L, int T) { return sizeof(double) * (size_t)k14_lds(kx, L, T).total; }

// ---------------------------------------------------------------- solve
__global__ void __launch_bounds__(64) k14_solve_kernel(const IvArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int lane = threadIdx.x, T = a.kt, nz = T + 1, ne = nz * (nz + 1) / 2;
    const int nf = a.n_feat, icpt = a.icpt, kx = nf + icpt, k1 = nf - a.n_endog, m = a.n_inst, L = kx - a.n_endog + m;
    const int LD = L + 1, LDB = kx + 1;
    const K14Lds o = k14_lds(kx, L, T);
    double *Gs = dyn + o.Gs, *A = dyn + o.A, *d0 = dyn + o.d0, *B = dyn + o.B, *Gm2 = dyn + o.Gm2, *A2 = dyn + o.A2, *rhs2 = dyn + o.rhs2,
           *d02 = dyn + o.d02, *Ri = dyn + o.Ri, *tmp = dyn + o.tmp;
    const int64_t g = blockIdx.x;
    // (fit_group_items, written out: through the call the compiler fetches the two seg_first words with one 8-byte scalar load and lays
    // the head of the kernel out differently, and the long-group lines of scripts/bench_iv.py -- one wave summing every segment's
    // partials -- came out up to 0.3 % over the range of the kernel before; this form compiles to that kernel's instructions up to
    // the inverse.  profiles/fit_group_stages_bench.txt has both runs; the second does not prove the helper was the cause)
    const int64_t v0 = a.seg_offs ? a.seg_first[g] : g, v1 = a.seg_offs ? a.seg_first[g + 1] : g + 1;
    const bool finite = fit_sum_parts(a.gram_part, k10_gram_stride(T), v0, v1, ne + 1, Gs, lane);   // the triangle, then n
    fit_wave_sync();
    const double n = Gs[ne];
    // where column i of X and column l of Z (factorisation order [X1 | 1 | Z2]) sit in the staged list [X1 | X2 | Z2 | 1]
    auto xg = [&](int i) { return i < nf ? i : T - 1; };
    auto zg = [&](int l) { return l < k1 ? l : (icpt && l == k1 ? T - 1 : nf + (l - k1 - icpt)); };
    auto S = [&](int p, int q) { const int i = p < q ? p : q, j = p < q ? q : p; return Gs[tri_index(i, j, nz)]; };
    bool ok = finite && n > (double)L;
    if (ok) {
        for (int p = lane; p < L * L; p += 64) {
            const int i = p / L, j = p - i * L;
            const double v = S(zg(i), zg(j));
            A[i * LD + j] = v;
            if (i == j) d0[i] = v;
        }
        for (int p = lane; p < L * LDB; p += 64) {
            const int l = p / LDB, c = p - l * LDB;
            B[l * LDB + c] = S(zg(l), c < kx ? xg(c) : T);
        }
        fit_wave_sync();
        ok = fit_chol_factor(A, d0, L, lane);
    }
    if (ok) {
        if (lane < LDB) {                                          // R [Q | r] = [C | Z~'y~]: lane c owns column c
            for (int j = 0; j < L; ++j) {
                double s = B[j * LDB + lane];
                for (int i = 0; i < j; ++i) s = fma(-A[j * LD + i], B[i * LDB + lane], s);
                B[j * LDB + lane] = s / A[j * LD + j];
            }
        }
        fit_wave_sync();
        for (int en = lane; en < (kx + 1) * (kx + 2) / 2; en += 64) {   // [Q | r]'[Q | r], packed as fit_chol_solve reads it
            int i, j;
            tri_unpack(en, LDB, i, j);
            double v = 0.0;
            for (int l = 0; l < L; ++l) v = fma(B[l * LDB + i], B[l * LDB + j], v);
            Gm2[en] = v;
        }
        fit_wave_sync();
        ok = fit_chol_solve(Gm2, A2, rhs2, d02, kx, lane);
    }
    double *st = a.state + (size_t)g * k14_state_stride(kx, L);
    double fsf = fit_nan(), pr2 = fit_nan();
    if (ok) {
        if (lane < L) {                                            // the Sargan terms r - Q b
            double v = B[lane * LDB + kx];
            for (int c = 0; c < kx; ++c) v = fma(-B[lane * LDB + c], rhs2[c], v);
            tmp[lane] = v * v;
        }
        if (lane < a.n_endog) {                                    // the first stage of endogenous column `lane`
            const int c = k1 + lane;
            double qq = 0.0, dl = 0.0;
            for (int l = 0; l < L; ++l) {
                const double q = B[l * LDB + c];
                qq = fma(q, q, qq);
                if (l >= L - m) dl = fma(q, q, dl);
            }
            const double rssu = S(c, c) - qq;
            fsf = (dl / (double)m) / (rssu / (n - (double)L));
            pr2 = dl / (dl + rssu);
        }
        fit_chol_inverse(A2, Ri, st + 4 + kx, kx, lane);           // M^-1 (its fit_wave_sync() publishes tmp as well)
        if (lane == 0) {
            double v = 0.0;
            for (int l = 0; l < L; ++l) v += tmp[l];
            st[2] = v;
        }
        if (lane < kx) {                                           // R'Pi = Q in place, rows stored in the tile's order [X1 | Z2 | 1]
            double *Pi = st + 4 + kx + kx * kx;
            for (int j = L - 1; j >= 0; --j) {
                double s = B[j * LDB + lane];
                for (int i = j + 1; i < L; ++i) s = fma(-A[i * LD + j], B[i * LDB + lane], s);
                s /= A[j * LD + j];
                B[j * LDB + lane] = s;
                const int row = j < k1 ? j : (icpt && j == k1 ? L - 1 : j - icpt);
                Pi[row * kx + lane] = s;
            }
        }
    }
    if (lane == 0) {
        st[0] = n;
        st[1] = ok ? 1.0 : 0.0;
        if (!ok) st[2] = fit_nan();
        st[3] = 0.0;
        if (a.status) a.status[g] = !(n > 0.0) ? POLS_GROUP_EMPTY : (!(n > (double)L) ? POLS_GROUP_BAD_DOF : (ok ? POLS_GROUP_OK : POLS_GROUP_FALLBACK));
        if (a.n_obs) a.n_obs[g] = (int64_t)n;
    }
    const double fillv = n > 0.0 ? fit_nan() : 0.0;                // no rows: zeros, as the existing entries
    if (lane < kx) {
        const double bv = ok ? rhs2[lane] : fillv;
        st[4 + lane] = bv;
        fit_store_coef(a, g, kx, lane, bv);
    }
    if (a.pred_all) {                                              // [b_X1 b_X2 | 0 (Z2) | b_1]
        if (lane < T) a.coefp[(size_t)g * T + lane] = lane < nf ? (ok ? rhs2[lane] : fillv) : (lane < nf + m ? 0.0 : (ok ? rhs2[nf] : fillv));
    } else if (lane < kx) {
        a.coefp[(size_t)g * kx + lane] = ok ? rhs2[lane] : fillv;
    }
    if (lane < a.n_endog) {
        if (a.first_stage_f) a.first_stage_f[(size_t)g * a.n_endog + lane] = fsf;
        if (a.partial_r2) a.partial_r2[(size_t)g * a.n_endog + lane] = pr2;
    }
}

int k14_solve_launch(pols_ctx *ctx, const IvArgs &a) {
    const int kx = a.n_feat + a.icpt, L = kx - a.n_endog + a.n_inst;
    return fit_launch_plain(ctx, k14_solve_kernel, a.n_groups, 64, k14_solve_lds(kx, L, a.kt), a);
}

// ---------------------------------------------------------------- rows
template <typename T, bool ROBUST>
__global__ void __launch_bounds__(256) k14_rows_kernel(const IvArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, TT = a.kt;
    const int nf = a.n_feat, icpt = a.icpt, kx = nf + icpt, k1 = nf - a.n_endog, L = kx - a.n_endog + a.n_inst;
    constexpr int ts = ROBUST ? FIT_TS : FIT_TILE;            // (robust: the parked columns are read across threads)
    double *xs = dyn;                                              // (T + 2) x ts
    double *us = xs + (size_t)(TT + 2) * ts;                       // ROBUST: kx x ts
    double *bs = us + (ROBUST ? (size_t)kx * ts : 0);              // kx
    double *Ps = bs + kx;                                          // ROBUST: L x kx
    double *red = Ps + (ROBUST ? L * kx : 0);                      // 4
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    const double *st = a.state + (size_t)g * k14_state_stride(kx, L);
    if (st[1] == 0.0) ntiles = 0;                                  // no fit: nothing to sum (workgroup-uniform)
    if (tid < kx) bs[tid] = st[4 + tid];
    if constexpr (ROBUST)
        for (int q = tid; q < L * kx; q += 256) Ps[q] = st[4 + kx + kx * kx + q];
    const TriSpread sp = tri_spread(kx, tid);                      // the kx (kx + 1) / 2 entries of sum u_i u_i'
    double acc[3] = {0.0, 0.0, 0.0};
    double rss = 0.0;
    __syncthreads();
    for (int64_t it = 0; it < ntiles; ++it) {
        const int64_t t0 = base + it * FIT_TILE;
        const bool fit = fit_stage<T, true>(a, s, e, t0, xs, ts);
        double f = 0.0;
        for (int i = 0; i < nf; ++i) f = fma(xs[(size_t)i * ts + tid], bs[i], f);
        if (icpt) f = fma(xs[(size_t)(TT - 1) * ts + tid], bs[nf], f);
        const double ev = fit ? xs[(size_t)TT * ts + tid] - f : 0.0;
        rss = fma(ev, ev, rss);
        if constexpr (ROBUST) {
            for (int c = 0; c < kx; ++c) {
                double xh = 0.0;
                for (int l = 0; l < L; ++l) xh = fma(Ps[l * kx + c], xs[(size_t)(l < k1 ? l : l + a.n_endog) * ts + tid], xh);
                us[(size_t)c * ts + tid] = fit ? ev * xh : 0.0;
            }
            __syncthreads();
            tri_accumulate(sp, acc, us, ts, 0, (int)min((int64_t)FIT_TILE, e - t0));
        }
        __syncthreads();                                           // the next tile overwrites xs and us
    }
    double *out = a.rows_part + (size_t)blockIdx.x * k14_rows_stride(kx, ROBUST);
    const double tot = fit_block_sum(rss, red, lane, wv);
    if (tid == 0) out[0] = tot;
    if constexpr (ROBUST) tri_reduce(sp, acc, xs, out + 1);
}

static size_t k14_rows_lds(int T, int kx, int L, bool robust) {
    return sizeof(double) * ((size_t)(T + 2) * (robust ? FIT_TS : FIT_TILE) + (robust ? (size_t)kx * FIT_TS + (size_t)L * kx : 0) + kx + 4);
}

template <typename T, bool ROBUST>
static int k14_rows_launch_t(pols_ctx *ctx, const IvArgs &a) {
    const int kx = a.n_feat + a.icpt, L = kx - a.n_endog + a.n_inst;
    const size_t lds = k14_rows_lds(a.kt, kx, L, ROBUST);
    if (lds > FIT_LDS_BUDGET) return fail(POLS_ERR_UNSUPPORTED, "iv2sls: %d columns exceed the LDS of a workgroup", a.kt);
    static OncePerDevice once;
    return fit_launch(ctx, &k14_rows_kernel<T, ROBUST>, once, fit_items(a), 256, lds, FIT_LDS_BUDGET, a);
}

int k14_rows_launch(pols_ctx *ctx, int dtype, const IvArgs &a) {
    if (a.n_groups == 0) return POLS_OK;
    const bool robust = a.cov_type != POLS_COV_NONROBUST;
    if (dtype == POLS_F32) return robust ? k14_rows_launch_t<float, true>(ctx, a) : k14_rows_launch_t<float, false>(ctx, a);
    return robust ? k14_rows_launch_t<double, true>(ctx, a) : k14_rows_launch_t<double, false>(ctx, a);
}

// ---------------------------------------------------------------- finish
__global__ void __launch_bounds__(64) k14_finish_kernel(const IvArgs a) {
    constexpr int KM = K14_TMAX - 1;                               // the most regressors: one instrument at least
    __shared__ double Mi[KM * KM], Me[KM * KM], W[KM * KM], rss_s;
    const int lane = threadIdx.x, kx = a.n_feat + a.icpt, L = kx - a.n_endog + a.n_inst, dof = a.n_inst - a.n_endog;
    const bool robust = a.cov_type != POLS_COV_NONROBUST;
    const int64_t g = blockIdx.x;
    int64_t v0, v1;
    fit_group_items(a, g, v0, v1);
    const double *st = a.state + (size_t)g * k14_state_stride(kx, L);
    const double n = st[0];
    const bool ok = st[1] != 0.0;                                  // (wave-uniform)
    double *cov = a.cov ? a.cov + (size_t)g * kx * kx : nullptr;
    if (!ok) {
        const double q = fit_nan();
        if (lane < kx) fit_store_stats(a, g, kx, lane, q, q, q);
        if (cov) for (int p = lane; p < kx * kx; p += 64) cov[p] = q;
        if (lane == 0) {
            if (a.sigma2) a.sigma2[g] = q;
            if (a.sargan) a.sargan[g] = q;
            if (a.sargan_p) a.sargan_p[g] = q;
        }
        return;
    }
    const size_t rs = k14_rows_stride(kx, robust);
    for (int en = lane; en < (int)rs; en += 64) {
        double v = 0.0;
        for (int64_t it = v0; it < v1; ++it) v += a.rows_part[(size_t)it * rs + en];
        if (en == 0) { rss_s = v; continue; }
        int i, j;
        tri_unpack(en - 1, kx, i, j);
        Me[i * kx + j] = v; Me[j * kx + i] = v;
    }
    for (int p = lane; p < kx * kx; p += 64) Mi[p] = st[4 + kx + p];
    __syncthreads();
    const double rss = rss_s;
    const double df = a.small_sample ? n - (double)kx : n;
    const double sigma2 = rss / df;
    if (robust) {
        for (int p = lane; p < kx * kx; p += 64) {
            const int i = p / kx, j = p - i * kx;
            double v = 0.0;
            for (int l = 0; l < kx; ++l) v = fma(Mi[i * kx + l], Me[l * kx + j], v);
            W[p] = v;
        }
        __syncthreads();
        const double scale = a.cov_type == POLS_COV_HC1 ? n / df : 1.0;
        for (int p = lane; p < kx * kx; p += 64) {
            const int i = p / kx, j = p - i * kx;
            double v = 0.0;
            for (int l = 0; l < kx; ++l) v = fma(W[i * kx + l], Mi[l * kx + j], v);
            Me[p] = v * scale;
        }
    } else {
        for (int p = lane; p < kx * kx; p += 64) Me[p] = sigma2 * Mi[p];
    }
    __syncthreads();
    if (cov) for (int p = lane; p < kx * kx; p += 64) cov[p] = Me[p];
    if (lane < kx) {
        // (not fit_se_t_p: on a NaN t it stores the canonical NaN, k7_betai its argument's -- one form for both would change bytes)
        const double se = sqrt(Me[lane * kx + lane]), tv = st[4 + lane] / se;
        const double pv = !a.p_values ? 0.0 : (a.small_sample ? k7_betai(0.5 * df, 0.5, df / (df + tv * tv)) : erfc(fabs(tv) * 0.70710678118654752440));
        fit_store_stats(a, g, kx, lane, se, tv, pv);
    }
    if (lane == 0) {
        if (a.sigma2) a.sigma2[g] = sigma2;
        const double sg = dof > 0 ? n * st[2] / rss : fit_nan();
        if (a.sargan) a.sargan[g] = sg;
        if (a.sargan_p) a.sargan_p[g] = dof > 0 ? k7_gammaq(0.5 * (double)dof, 0.5 * sg) : fit_nan();
    }
}

int k14_finish_launch(pols_ctx *ctx, const IvArgs &a) { return fit_launch_plain(ctx, k14_finish_kernel, a.n_groups, 64, 0, a); }

}  // namespace pols
