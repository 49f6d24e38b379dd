// k18_glsar.hip -- K18: AR(1) feasible GLS per group, Cochrane-Orcutt / Prais-Winsten (pols_glsar).
//
// Per group g, the rows in frame order t = 1..n (time order; every row is a fitted row: "ignore" or "zero"), z_t = (x_t | 1 | y_t),
// T = kt + 1 columns.  Moments, one pass over the columns:
//   S = sum_{1..n} z_t z_t',  C = sum_{2..n} z_t z_{t-1}',  S_1 = S - z_1 z_1',  S_n = S - z_n z_n'.
// The transformed rows at rho are z*_t = z_t - rho z_{t-1} (t >= 2), Prais-Winsten adds z*_1 = sqrt(1 - rho^2) z_1; their cross-moments are
//   A(rho) = S_1 - rho (C + C') + rho^2 S_n  [+ (1 - rho^2) z_1 z_1'],
// b(rho) solves the X-block of A(rho) against its y-column (fit_chol_solve: a pivot fails when d^2 <= 16 kt eps A_jj).
// Iteration: rho^0 = 0 (b^0 is OLS); v = (-b^i, 1): rho^{i+1} = v'C v / v'S_n v (e_t on e_{t-1} over t = 2..n, e on the original rows);
// stop when |rho^{i+1} - rho^i| <= tol or after max_iter updates (NOT_CONVERGED, the result is still returned); the reported b is
// b(rho*) at the last rho -- one more solve.  Reported: e_t = y_t - x_t'b, u_t = e_t - rho* e_{t-1} (t >= 2), u_1 = sqrt(1 - rho*^2) e_1
// (Prais-Winsten); RSS* = sum u^2 SUMMED OVER THE ROWS, df = n* - kt, V = RSS* / df A_xx(rho*)^-1, dw = sum (u_t - u_{t-1})^2 / RSS*,
// dw_ols the same of e0 = y - X b^0.  Everything is f64 on the inputs' values, for f32 batches too.  No atomics, every sum in a fixed
// order: two runs are bit-identical.
//
// Launches (one workgroup per segment of a long group -- ensure_segments -- or per group, unless said otherwise):
//   lag_gram  256-row tiles staged by fit_stage at row index 1 of every column: index 0 holds the row before the tile (the carry: the
//             last row of the tile before, or -- first tile of a segment that does not start its group -- row s - 1 read straight from
//             the columns; rows of the grid before s are zero, so the slot of row s - 1 is always written).  The packed triangle of S
//             goes through tri_spread / tri_accumulate / tri_reduce, the T x T entries of C are spread the same way (row partitions
//             below 256 entries, up to four entries per thread beyond) and accumulated as c_i[r] c_j[r - 1] over the item's rows.
//   solve     one wave per group: the partials summed in segment order (a non-finite moment fails the group), z_1 and z_n read from
//             the columns, then the whole iteration in LDS: A(rho) packed as fit_chol_solve reads it, the solve, lane i's row of v'C v
//             and v'S_n v, their sums in lane order.  b, b^0, rho*, A_xx(rho*)^-1 go to the group's state; coef, rho, n_iter, n_obs
//             and status are final here.
//   rows      only when se / t / p / cov / sigma2 / dw / dw_ols is wanted: the thread of a row computes e and e0 and parks them beside
//             two carried values (e_{t-1}, e_{t-2} across tiles; rows s - 1 and s - 2 read straight from the columns at a segment
//             start), then adds its terms of RSS*, sum (du)^2, sum (de0)^2 and sum e0^2; tiles in order, DPP within a wave, the waves
//             as (0 + 1) + (2 + 3).
//   finish    one wave per group: the items' partials summed in order, sigma2, V, se / t / p, dw, dw_ols.
//   predict   K10's prediction launch from the f64 coefficients (api_fits.hip).
#include "k18_glsar.hpp"
#include "fit_launch.hpp"
#include "fit_group.inl"
#include "fit_lds.hpp"

namespace pols {

// column c of z at row r as fit_stage leaves it: a feature (null-filled unless "ignore"), the ones column, y at c = kt
template <typename T>
__device__ __forceinline__ double k18_value(const GlsarArgs &a, const int c, const int64_t r) {
    const int ku = a.k_user;
    if (c >= ku && c < a.kt) return 1.0;
    const void *col = a.y;                                         // (a run-time index into the kernel arguments would put them in scratch)
#pragma unroll
    for (int j = 0; j < POLS_MAX_FEATURES; ++j) col = (j == c && j < ku) ? a.x[j] : col;
    return (double)null_fill<T>(a.null_policy, static_cast<const T *>(col)[r]);
}

// ---------------------------------------------------------------- lag gram
template <typename T>
__global__ void __launch_bounds__(256) k18_lag_gram_kernel(const GlsarArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    double *xs = dyn;                                              // (kt + 2) x FIT_TS: index 0 of a column the row before the tile, 1 .. 256 the tile
    const int tid = threadIdx.x, kt = a.kt, TT = kt + 1, ne = TT * (TT + 1) / 2, nc = TT * TT;
    const int ts = FIT_TS;
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    const int64_t g0 = a.offs[g];
    const TriSpread sp = tri_spread(TT, tid);
    // the T x T entries of C: entry en = i T + j pairs column i at row r with column j at row r - 1
    const int cparts = nc < 256 ? 256 / nc : 1;
    const int cpart = cparts > 1 ? tid / nc : 0;
    int ci[4], cj[4];
    bool con[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int en = cparts > 1 ? tid - cpart * nc : tid + 256 * q;
        con[q] = cparts > 1 ? (q == 0 && cpart < cparts) : en < nc;
        const int en0 = con[q] ? en : 0;
        ci[q] = en0 / TT;
        cj[q] = en0 - ci[q] * TT;
    }
    double acc[3] = {0.0, 0.0, 0.0}, cacc[4] = {0.0, 0.0, 0.0, 0.0};
    int nfit = 0;
    for (int64_t it = 0; it < ntiles; ++it) {
        const int64_t t0 = base + it * FIT_TILE;
        nfit += fit_stage<T, false>(a, s, e, t0, xs + 1, ts) ? 1 : 0;
        if (it == 0) {                                             // the row before the item: of this group, or nothing
            if (tid < TT) xs[(size_t)tid * ts + (int)(s - t0)] = s > g0 ? k18_value<T>(a, tid, s - 1) : 0.0;
            __syncthreads();
        }
        const int q0 = (int)max(s - t0, (int64_t)0) + 1, q1 = (int)min((int64_t)FIT_TILE, e - t0) + 1;
        tri_accumulate(sp, acc, xs, ts, q0, q1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!con[q]) continue;
            const double *pi = xs + (size_t)ci[q] * ts, *pj = xs + (size_t)cj[q] * ts - 1;
            double v = cacc[q];
            for (int r = q0 + cpart; r < q1; r += cparts) v = fma(pi[r], pj[r], v);
            cacc[q] = v;
        }
        const double carry = tid < TT ? xs[(size_t)tid * ts + FIT_TILE] : 0.0;
        __syncthreads();                                           // the next tile overwrites xs
        if (tid < TT) xs[(size_t)tid * ts] = carry;
    }
    double *out = a.gram_part + (size_t)blockIdx.x * k18_gram_stride(kt);
    tri_reduce(sp, acc, xs, out);
    if (cparts > 1) {
        if (con[0]) xs[tid] = cacc[0];                             // (tid = part nc + entry)
        __syncthreads();
        if (tid < nc) {
            double v = 0.0;
            for (int p = 0; p < cparts; ++p) v += xs[p * nc + tid];
            out[ne + tid] = v;
        }
        __syncthreads();
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (con[q]) out[ne + tid + 256 * q] = cacc[q];
    }
    xs[tid] = (double)nfit;
    __syncthreads();
    if (tid == 0) {
        double v = 0.0;
        for (int t = 0; t < 256; ++t) v += xs[t];
        out[ne + nc] = v;
    }
}

size_t k18_gram_lds(int kt) { return sizeof(double) * (size_t)(kt + 2) * FIT_TS; }

template <typename T>
static int k18_gram_launch_t(pols_ctx *ctx, const GlsarArgs &a) {
    static OncePerDevice once;
    return fit_launch(ctx, &k18_lag_gram_kernel<T>, once, fit_items(a), 256, k18_gram_lds(a.kt), FIT_LDS_BUDGET, a);
}

int k18_gram_launch(pols_ctx *ctx, int dtype, const GlsarArgs &a) {
    if (a.kt < 1 || a.kt > K18_KMAX) return fail(POLS_ERR_UNSUPPORTED, "glsar: %d features (incl. intercept) outside 1..%d", a.kt, K18_KMAX);
    if (a.n_groups == 0) return POLS_OK;
    return dtype == POLS_F32 ? k18_gram_launch_t<float>(ctx, a) : k18_gram_launch_t<double>(ctx, a);
}

// ---------------------------------------------------------------- solve
size_t k18_solve_lds(int kt) { return sizeof(double) * (size_t)k18_lds(kt).total; }

template <typename T>
__global__ void __launch_bounds__(64) k18_solve_kernel(const GlsarArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int lane = threadIdx.x, kt = a.kt, TT = kt + 1, ne = TT * (TT + 1) / 2, nc = TT * TT;
    const K18Lds o = k18_lds(kt);
    double *Ss = dyn + o.Ss, *Cs = dyn + o.Cs, *z1 = dyn + o.z1, *zn = dyn + o.zn, *Gm = dyn + o.Gm, *A = dyn + o.A, *rhs = dyn + o.rhs,
           *d0 = dyn + o.d0, *b0 = dyn + o.b0, *vv = dyn + o.vv, *tn = dyn + o.tn, *td = dyn + o.td, *Ri = dyn + o.Ri;
    int32_t *ij = reinterpret_cast<int32_t *>(dyn + o.ij);
    const int64_t g = blockIdx.x;
    int64_t v0, v1;
    fit_group_items(a, g, v0, v1);
    const int64_t r0 = a.offs[g], r1 = a.offs[g + 1];
    const bool pw = a.method == POLS_AR1_PRAIS_WINSTEN;
    // S and, right behind it in the partials as in LDS, C (the row count that follows them is not read: every row is a fitted row)
    const bool finite = fit_sum_parts(a.gram_part, k18_gram_stride(kt), v0, v1, ne + nc, Ss, lane);
    for (int en = lane; en < ne; en += 64) {
        int i, j;
        tri_unpack(en, TT, i, j);
        ij[en] = i << 8 | j;
    }
    const double n = (double)(r1 - r0);                            // (every row is a fitted row)
    if (lane < TT) {
        z1[lane] = r1 > r0 ? k18_value<T>(a, lane, r0) : 0.0;
        zn[lane] = r1 > r0 ? k18_value<T>(a, lane, r1 - 1) : 0.0;
    }
    fit_wave_sync();
    const double nstar = pw ? n : n - 1.0;
    const bool dof = nstar > (double)kt;
    bool ok = finite && dof;
    double rho = 0.0;
    int n_iter = 0;
    bool conv = false;
    while (ok) {
        const double r2 = rho * rho, head = pw ? 1.0 - r2 : 0.0;
        for (int en = lane; en < ne; en += 64) {
            const int i = ij[en] >> 8, j = ij[en] & 255;
            const double sij = Ss[en], f = z1[i] * z1[j], l = zn[i] * zn[j];
            double v = (sij - f) - rho * (Cs[i * TT + j] + Cs[j * TT + i]) + r2 * (sij - l);
            if (pw) v = fma(head, f, v);
            Gm[en] = v;
        }
        fit_wave_sync();
        ok = fit_chol_solve(Gm, A, rhs, d0, kt, lane);
        if (!ok) break;
        if (n_iter == 0 && lane < kt) b0[lane] = rhs[lane];
        if (conv || n_iter == a.max_iter) break;
        if (lane < TT) vv[lane] = lane < kt ? -rhs[lane] : 1.0;
        fit_wave_sync();
        if (lane < TT) {                                           // row `lane` of v'C v and of v'S_n v
            double sn = 0.0, sd = 0.0;
            for (int j = 0; j < TT; ++j) {
                const int lo = lane < j ? lane : j, hi = lane < j ? j : lane;
                sn = fma(Cs[lane * TT + j], vv[j], sn);
                sd = fma(Ss[tri_index(lo, hi, TT)] - zn[lane] * zn[j], vv[j], sd);
            }
            tn[lane] = vv[lane] * sn;
            td[lane] = vv[lane] * sd;
        }
        fit_wave_sync();
        double num = 0.0, den = 0.0;
        for (int i = 0; i < TT; ++i) { num += tn[i]; den += td[i]; }   // (every lane the same words, the same order)
        fit_wave_sync();
        ++n_iter;
        const double next = num / den;
        if (!(den > 0.0 && den <= FIT_DBL_MAX) || !(fabs(next) < 1.0)) { ok = false; break; }
        conv = fabs(next - rho) <= a.tol;
        rho = next;
    }
    double *st = a.state + (size_t)g * k18_state_stride(kt);
    if (ok) fit_chol_inverse(A, Ri, st + 4 + 2 * kt, kt, lane);    // A_xx(rho*)^-1
    if (lane == 0) {
        st[0] = n;
        st[1] = ok ? 1.0 : 0.0;
        st[2] = ok ? rho : fit_nan();
        st[3] = ok ? sqrt(1.0 - rho * rho) : fit_nan();
        if (a.status)
            a.status[g] = !(n > 0.0) ? POLS_GROUP_EMPTY : (!dof ? POLS_GROUP_BAD_DOF : (!ok ? POLS_GROUP_FALLBACK : (conv ? POLS_GROUP_OK : POLS_GROUP_NOT_CONVERGED)));
        if (a.n_obs) a.n_obs[g] = r1 - r0;
        if (a.rho) a.rho[g] = ok ? rho : fit_nan();
        if (a.n_iter) a.n_iter[g] = n_iter;
    }
    const double fillv = n > 0.0 ? fit_nan() : 0.0;                // no rows: zeros, as the existing entries
    if (lane < kt) {
        const double bv = ok ? rhs[lane] : fillv;
        st[4 + lane] = bv;
        st[4 + kt + lane] = ok ? b0[lane] : fillv;
        a.coefp[(size_t)g * kt + lane] = bv;
        fit_store_coef(a, g, kt, lane, bv);
    }
}

int k18_solve_launch(pols_ctx *ctx, int dtype, const GlsarArgs &a) {
    const size_t lds = k18_solve_lds(a.kt);
    return dtype == POLS_F32 ? fit_launch_plain(ctx, k18_solve_kernel<float>, a.n_groups, 64, lds, a)
                             : fit_launch_plain(ctx, k18_solve_kernel<double>, a.n_groups, 64, lds, a);
}

// ---------------------------------------------------------------- rows
template <typename T>
__global__ void __launch_bounds__(256) k18_rows_kernel(const GlsarArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, kt = a.kt, TT = kt + 1;
    constexpr int ts = FIT_TILE;
    double *xs = dyn;                                              // (kt + 2) x ts
    double *E = xs + (size_t)(kt + 2) * ts;                        // 2 + 256: e of rows t0 - 2, t0 - 1, then of the tile
    double *E0 = E + 2 + FIT_TILE;                                 // the same of e0
    double *bs = E0 + 2 + FIT_TILE;                                // kt
    double *b0s = bs + kt;                                         // kt
    double *zp = b0s + kt;                                         // 2 x T: rows s - 1 and s - 2
    double *prev = zp + 2 * TT;                                    // e(s - 1), e(s - 2), e0(s - 1), e0(s - 2)
    double *red = prev + 4;                                        // 4
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    const int64_t g0 = a.offs[g];
    const double *st = a.state + (size_t)g * k18_state_stride(kt);
    if (st[1] == 0.0) ntiles = 0;                                  // no fit: nothing to sum (workgroup-uniform)
    const double rho = st[2], head = st[3];
    const bool pw = a.method == POLS_AR1_PRAIS_WINSTEN;
    if (tid < kt) { bs[tid] = st[4 + tid]; b0s[tid] = st[4 + kt + tid]; }
    if (tid < 2 * TT) {
        const int back = tid / TT, c = tid - back * TT;
        const int64_t r = s - 1 - back;
        zp[tid] = (ntiles > 0 && r >= g0) ? k18_value<T>(a, c, r) : 0.0;
    }
    __syncthreads();
    if (tid < 2) {
        const double *z = zp + tid * TT;
        double f = 0.0, f0 = 0.0;
        for (int i = 0; i < kt; ++i) { f = fma(z[i], bs[i], f); f0 = fma(z[i], b0s[i], f0); }
        prev[tid] = z[kt] - f;
        prev[2 + tid] = z[kt] - f0;
    }
    __syncthreads();
    double rss = 0.0, dwn = 0.0, d0n = 0.0, s0 = 0.0;
    for (int64_t it = 0; it < ntiles; ++it) {
        const int64_t t0 = base + it * FIT_TILE;
        const bool fit = fit_stage<T, true>(a, s, e, t0, xs, ts);
        double f = 0.0, f0 = 0.0;
        for (int i = 0; i < kt; ++i) {                             // (features, then the ones column: the staged order)
            const double x = xs[(size_t)i * ts + tid];
            f = fma(x, bs[i], f);
            f0 = fma(x, b0s[i], f0);
        }
        const int64_t row = t0 + tid;
        double ev = fit ? xs[(size_t)kt * ts + tid] - f : 0.0, e0v = fit ? xs[(size_t)kt * ts + tid] - f0 : 0.0;
        if (it == 0) {                                             // rows s - 1 and s - 2: inside the tile grid, or in the two slots before it
            if (row == s - 1) { ev = prev[0]; e0v = prev[2]; }
            if (row == s - 2) { ev = prev[1]; e0v = prev[3]; }
            if (tid < 2) {
                const int64_t r = t0 - 2 + tid;
                E[tid] = r == s - 1 ? prev[0] : (r == s - 2 ? prev[1] : 0.0);
                E0[tid] = r == s - 1 ? prev[2] : (r == s - 2 ? prev[3] : 0.0);
            }
        }
        E[2 + tid] = ev;
        E0[2 + tid] = e0v;
        __syncthreads();
        if (fit) {
            const int64_t t = row - g0;                            // 0 for the group's first row
            const double e1 = E[1 + tid], e2 = E[tid];
            s0 = fma(e0v, e0v, s0);
            if (t >= 1) {
                const double u = ev - rho * e1, d = e0v - E0[1 + tid];
                rss = fma(u, u, rss);
                d0n = fma(d, d, d0n);
                if (t >= 2 || pw) {
                    const double du = u - (t >= 2 ? e1 - rho * e2 : head * e1);
                    dwn = fma(du, du, dwn);
                }
            } else if (pw) {
                const double u = head * ev;
                rss = fma(u, u, rss);
            }
        }
        const double c = tid < 2 ? E[FIT_TILE + tid] : 0.0, c0 = tid < 2 ? E0[FIT_TILE + tid] : 0.0;
        __syncthreads();                                           // the next tile overwrites xs, E and E0
        if (tid < 2) { E[tid] = c; E0[tid] = c0; }
    }
    double *out = a.rows_part + (size_t)blockIdx.x * K18_ROWS_STRIDE;
    const double t_rss = fit_block_sum(rss, red, lane, wv), t_dw = fit_block_sum(dwn, red, lane, wv);
    const double t_d0 = fit_block_sum(d0n, red, lane, wv), t_s0 = fit_block_sum(s0, red, lane, wv);
    if (tid == 0) { out[0] = t_rss; out[1] = t_dw; out[2] = t_d0; out[3] = t_s0; }
}

static size_t k18_rows_lds(int kt) {
    return sizeof(double) * ((size_t)(kt + 2) * FIT_TILE + 2 * (2 + FIT_TILE) + 2 * (size_t)kt + 2 * (size_t)(kt + 1) + 4 + 4);
}

template <typename T>
static int k18_rows_launch_t(pols_ctx *ctx, const GlsarArgs &a) {
    static OncePerDevice once;
    return fit_launch(ctx, &k18_rows_kernel<T>, once, fit_items(a), 256, k18_rows_lds(a.kt), FIT_LDS_BUDGET, a);
}

int k18_rows_launch(pols_ctx *ctx, int dtype, const GlsarArgs &a) {
    if (a.n_groups == 0) return POLS_OK;
    return dtype == POLS_F32 ? k18_rows_launch_t<float>(ctx, a) : k18_rows_launch_t<double>(ctx, a);
}

// ---------------------------------------------------------------- finish
__global__ void __launch_bounds__(64) k18_finish_kernel(const GlsarArgs a) {
    const int lane = threadIdx.x, kt = a.kt;
    const int64_t g = blockIdx.x;
    int64_t v0, v1;
    fit_group_items(a, g, v0, v1);
    const double *st = a.state + (size_t)g * k18_state_stride(kt);
    const double n = st[0];
    const bool ok = st[1] != 0.0;                                  // (wave-uniform)
    double *cov = a.cov ? a.cov + (size_t)g * kt * kt : nullptr;
    double sums[K18_ROWS_STRIDE] = {0.0, 0.0, 0.0, 0.0};           // (every lane the same words, the same order)
    if (ok)
        for (int64_t it = v0; it < v1; ++it)
#pragma unroll
            for (int q = 0; q < (int)K18_ROWS_STRIDE; ++q) sums[q] += a.rows_part[(size_t)it * K18_ROWS_STRIDE + q];
    const double q = fit_nan();
    const double df = (a.method == POLS_AR1_PRAIS_WINSTEN ? n : n - 1.0) - (double)kt;
    const double sigma2 = ok ? sums[0] / df : q;
    const double *Ai = st + 4 + 2 * kt;
    if (cov) for (int p = lane; p < kt * kt; p += 64) cov[p] = ok ? sigma2 * Ai[p] : q;
    if (lane < kt) {
        // (not fit_se_t_p: on a NaN t it stores the canonical NaN, k7_betai its argument's -- one form for both would change bytes)
        const double se = ok ? sqrt(sigma2 * Ai[lane * kt + lane]) : q, tv = ok ? st[4 + lane] / se : q;
        fit_store_stats(a, g, kt, lane, se, tv, (ok && a.p_values) ? k7_betai(0.5 * df, 0.5, df / (df + tv * tv)) : q);
    }
    if (lane == 0) {
        if (a.sigma2) a.sigma2[g] = sigma2;
        if (a.dw) a.dw[g] = ok ? sums[1] / sums[0] : q;
        if (a.dw_ols) a.dw_ols[g] = ok ? sums[2] / sums[3] : q;
    }
}

int k18_finish_launch(pols_ctx *ctx, const GlsarArgs &a) { return fit_launch_plain(ctx, k18_finish_kernel, a.n_groups, 64, 0, a); }

}  // namespace pols
