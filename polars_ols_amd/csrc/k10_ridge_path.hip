// k10_ridge_path.hip -- K10: ridge regularisation path with closed-form leave-one-out selection (pols_ridge_cv).
//
// Per group g, on the rows F_g that pols_least_squares fits (null policy, sqrt(w) scaling with a null weight acting as 1e-24, ones
// column last and penalised like any other), x~_i = sqrt(w_i) x_i, y~_i = sqrt(w_i) y_i, n = |F_g|, and for every candidate a_j:
//   A_j = X~'X~ + a_j I,  b_j = A_j^-1 X~'y~,  h_ij = x~_i' A_j^-1 x~_i,
//   cv_scores[g][j] = (1 / n) sum_{i in F_g} ((y~_i - x~_i'b_j) / (1 - h_ij))^2      (the exact leave-one-out error of that ridge)
// One symmetric eigendecomposition X~'X~ = V diag(s) V' serves every candidate: with z_i = V'x~_i, c = V'X~'y~, d_m = 1 / (s_m + a_j):
//   h_ij = sum_m z_im^2 d_m,   x~_i'b_j = sum_m z_im c_m d_m,   b_j = V (d o c).
// USABILITY, the rule actually applied.  Candidate j is unusable for a group (NaN score, NaN coef_path row) when
//   * min(s) + a_j <= 16 kt eps (max(s) + a_j) in the computed spectrum -- "A_j has no Cholesky factorisation": the noise floor is the
//     one fix_chol_solve puts on a pivot, rounding noise around the exact 0 of a singular matrix fails rather than flips a coin; or
//   * some fitted row has 1 - h_ij < 1e-10 (K7r's HC2 / HC3 rule), or the score is not a number (NaNs under "ignore").
// Everything is f64 on the inputs' values, for f32 batches too.  No atomics, every sum in a fixed order: two runs are bit-identical.
//
// Launches (one workgroup per segment of a long group -- ensure_segments -- or per group, unless said otherwise):
//   gram   256-row tiles of the columns go to LDS as f64 with the null policy and sqrt(w) applied (fit_stage, fit_tile.inl).  The
//          (kt + 1)(kt + 2) / 2 entries of [X~ | y~]'[X~ | y~] are spread over the threads (tri_spread): with few entries several row
//          partitions per entry (summed in partition order at the end), beyond 256 entries up to three per thread.  The tile's
//          column stride is odd, so the lanes of a wave -- different columns, the same row -- hit different banks.
//   eig    one wave per group: the segments' Gram matrices summed in segment order, cyclic Jacobi rotations on A and V in LDS (lane l
//          owns column l in the column step and row l in the row step), stops when the off-diagonal mass is below 1e-30 of the diagonal's.
//   rows   the same tiles again (streaming loads); the thread of a row computes z_i = V'x~_i once -- KT = 1 .. 16: unrolled, x~_i, z^2 and
//          z c in registers; 17 .. 31: parked in LDS -- then every candidate costs 2 kt FMAs against the table 1 / (s_m + a_j) read at
//          the same LDS address by every lane (a broadcast).  A wave sums a tile's terms by DPP and lane 63 adds them to the wave's own
//          slot of the candidate: tiles in order, waves ((0 + 1) + (2 + 3)).
//   pick   one wave per group, lane j = candidate j: segment sums in order, / n, usability, the winner (smallest score, lowest index
//          on a tie), b = V (d o c) of every candidate (coef_path) and of the winner (coef, and in f64 for the prediction pass), status.
//   predict  pred = x_i'b, resid = y_i - pred with the winner's coefficients, over every row of the frame as pols_least_squares leaves
//          them: features zero-filled under every policy but "ignore", "drop" masks the rows outside the fit, a zero weight gives NaN
//          (the reference's (sqrt(w) x)'b / sqrt(w)).  The walk is fit_predict_rows (fit_tile.inl): sums in f64, rounds once -- an f32
//          prediction is the f64 one to half an ulp.
#include "k10_ridge_path.hpp"
#include "fit_launch.hpp"
#include "fit_tile.inl"

namespace pols {

// ---------------------------------------------------------------- gram
// tri_spread (fit_tile.inl) into plain arrays, and below its accumulate and reduce steps written out.  This launch is most of
// pols_ridge_cv and of pols_iv2sls's coefficients; through TriSpread, tri_accumulate and tri_reduce the compiler orders the kernel's
// argument loads and parks its scalars differently (50 VGPRs for 52), and both entries measured 0.4 - 2.6 % slower.
__device__ __forceinline__ void k10_entries(const int nz, const int parts, const int part, int (&ei)[3], int (&ej)[3], bool (&on)[3]) {
    const int tid = threadIdx.x, ne = nz * (nz + 1) / 2;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int en = parts > 1 ? tid - part * ne : tid + 256 * q;
        on[q] = parts > 1 ? (q == 0 && part < parts) : en < ne;
        tri_unpack(on[q] ? en : 0, nz, ei[q], ej[q]);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) k10_gram_kernel(const RidgeCvArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    double *xs = dyn;                                              // (kt + 2) x FIT_TS
    const int tid = threadIdx.x, kt = a.kt, nz = kt + 1, ne = nz * (nz + 1) / 2;
    const int ts = FIT_TS;
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    const int parts = ne < 256 ? 256 / ne : 1;
    const int part = parts > 1 ? tid / ne : 0;
    int ei[3], ej[3];
    bool on[3];
    k10_entries(nz, parts, part, ei, ej, on);
    double acc[3] = {0.0, 0.0, 0.0};
    int nfit = 0;
    for (int64_t it = 0; it < ntiles; ++it) {
        const int64_t t0 = base + it * FIT_TILE;
        nfit += fit_stage<T, false>(a, s, e, t0, xs, ts) ? 1 : 0;
        const int rows_here = (int)min((int64_t)FIT_TILE, e - t0);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (!on[q]) continue;
            const double *ci = xs + (size_t)ei[q] * ts, *cj = xs + (size_t)ej[q] * ts;
            double v = acc[q];
            for (int r = part; r < rows_here; r += parts) v = fma(ci[r], cj[r], v);
            acc[q] = v;
        }
        __syncthreads();                                           // the next tile overwrites xs
    }
    double *out = a.gram_part + (size_t)blockIdx.x * k10_gram_stride(kt);
    if (parts > 1) {
        if (on[0]) xs[part * ne + (tid - part * ne)] = acc[0];
        __syncthreads();
        if (tid < ne) {
            double v = 0.0;
            for (int p = 0; p < parts; ++p) v += xs[p * ne + tid];
            out[tid] = v;
        }
        __syncthreads();
    } else {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (on[q]) out[tid + 256 * q] = acc[q];
    }
    xs[tid] = (double)nfit;
    __syncthreads();
    if (tid == 0) {
        double v = 0.0;
        for (int t = 0; t < 256; ++t) v += xs[t];
        out[ne] = v;
    }
}

static size_t k10_gram_lds(int kt) { return sizeof(double) * (size_t)(kt + 2) * FIT_TS; }

template <typename T>
static int k10_gram_launch_t(pols_ctx *ctx, const RidgeCvArgs &a) {
    static OncePerDevice once;
    return fit_launch(ctx, &k10_gram_kernel<T>, once, fit_items(a), 256, k10_gram_lds(a.kt), FIT_LDS_BUDGET, a);
}

int k10_gram_launch(pols_ctx *ctx, int dtype, const RidgeCvArgs &a) {
    if (a.kt < 1 || a.kt > K10_KMAX) return fail(POLS_ERR_UNSUPPORTED, "ridge_cv: %d features (incl. intercept) outside 1..%d", a.kt, K10_KMAX);
    if (a.n_groups == 0) return POLS_OK;
    return dtype == POLS_F32 ? k10_gram_launch_t<float>(ctx, a) : k10_gram_launch_t<double>(ctx, a);
}

// ---------------------------------------------------------------- eig
__global__ void __launch_bounds__(64) k10_eig_kernel(const RidgeCvArgs a) {
    constexpr int LD = K10_KMAX + 1;
    __shared__ double A[K10_KMAX * LD], Vm[K10_KMAX * LD], gy[K10_KMAX];
    const int lane = threadIdx.x, kt = a.kt, nz = kt + 1, ne = nz * (nz + 1) / 2;
    const int64_t g = blockIdx.x;
    const int64_t v0 = a.seg_offs ? a.seg_first[g] : g, v1 = a.seg_offs ? a.seg_first[g + 1] : g + 1;
    const size_t gs = k10_gram_stride(kt);
    double *E = a.eig + (size_t)g * k10_eig_stride(kt);
    for (int en = lane; en <= ne; en += 64) {
        double v = 0.0;
        for (int64_t it = v0; it < v1; ++it) v += a.gram_part[(size_t)it * gs + en];
        if (en == ne) { E[kt * kt + 2 * kt] = v; continue; }       // the group's fitted rows
        int i, j;
        tri_unpack(en, nz, i, j);
        if (j == kt) { if (i < kt) gy[i] = v; }
        else { A[i * LD + j] = v; A[j * LD + i] = v; }
    }
    for (int q = lane; q < kt * kt; q += 64) { const int i = q / kt, j = q - i * kt; Vm[i * LD + j] = i == j ? 1.0 : 0.0; }
    __syncthreads();
    const bool mine = lane < kt;
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0, dg = 0.0;
        if (mine) {
            for (int j = 0; j < kt; ++j) { const double v = A[lane * LD + j]; if (j == lane) dg = v * v; else off = fma(v, v, off); }
        }
        off = readlane63(wave_sum_row3(off));
        dg = readlane63(wave_sum_row3(dg));
        if (!(off > 1e-30 * dg)) break;                            // converged (or NaN data: nothing to converge to)
        for (int p = 0; p < kt - 1; ++p)
            for (int q = p + 1; q < kt; ++q) {
                const double apq = A[p * LD + q];
                if (apq == 0.0) continue;                          // (wave-uniform: every lane read the same word)
                const double app = A[p * LD + p], aqq = A[q * LD + q];
                const double th = (aqq - app) / (2.0 * apq);
                const double t = copysign(1.0, th) / (fabs(th) + sqrt(fma(th, th, 1.0)));
                const double c = 1.0 / sqrt(fma(t, t, 1.0)), sn = t * c;
                __syncthreads();                                   // every lane holds the rotation before A changes
                if (mine) {                                        // columns p, q of A and V, row `lane`
                    const double x = A[lane * LD + p], y = A[lane * LD + q];
                    A[lane * LD + p] = c * x - sn * y;
                    A[lane * LD + q] = sn * x + c * y;
                    const double u = Vm[lane * LD + p], w = Vm[lane * LD + q];
                    Vm[lane * LD + p] = c * u - sn * w;
                    Vm[lane * LD + q] = sn * u + c * w;
                }
                __syncthreads();
                if (mine) {                                        // rows p, q of A, column `lane`
                    const double x = A[p * LD + lane], y = A[q * LD + lane];
                    A[p * LD + lane] = c * x - sn * y;
                    A[q * LD + lane] = sn * x + c * y;
                }
                __syncthreads();
                if (lane == 0) { A[p * LD + q] = 0.0; A[q * LD + p] = 0.0; }
                __syncthreads();
            }
    }
    __syncthreads();
    for (int q = lane; q < kt * kt; q += 64) { const int i = q / kt, m = q - i * kt; E[q] = Vm[i * LD + m]; }
    if (mine) {
        E[kt * kt + lane] = A[lane * LD + lane];
        double cm = 0.0;
        for (int i = 0; i < kt; ++i) cm = fma(Vm[i * LD + lane], gy[i], cm);
        E[kt * kt + kt + lane] = cm;
    }
}

int k10_eig_launch(pols_ctx *ctx, const RidgeCvArgs &a) {
    if (a.n_groups == 0) return POLS_OK;
    hipLaunchKernelGGL(k10_eig_kernel, dim3((unsigned)a.n_groups), dim3(64), 0, ctx->stream, a);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

// ---------------------------------------------------------------- rows
// KT > 0: the unrolled build of exactly KT columns; KT == 0: run-time kt (17 .. 31), z^2 and z c parked in LDS
template <typename T, int KT>
__global__ void __launch_bounds__(256) k10_rows_kernel(const RidgeCvArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, kt = KT > 0 ? KT : a.kt, na = a.n_alphas;
    constexpr int ts = FIT_TILE;
    double *xs = dyn;                                              // (kt + 2) x 256
    double *zs = xs + (size_t)(kt + 2) * ts;                       // KT == 0: kt x 256
    double *Vs = zs + (KT > 0 ? 0 : (size_t)kt * ts);              // kt x kt
    double *cs = Vs + kt * kt;                                     // kt
    double *D = cs + kt;                                           // na x kt: 1 / (s_m + a_j)
    double *red = D + na * kt;                                     // na x 4
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    {
        const double *E = a.eig + (size_t)g * k10_eig_stride(kt);
        for (int q = tid; q < kt * kt; q += 256) Vs[q] = E[q];
        if (tid < kt) cs[tid] = E[kt * kt + kt + tid];
        for (int q = tid; q < na * kt; q += 256) { const int j = q / kt, m = q - j * kt; D[q] = 1.0 / (E[kt * kt + m] + a.alphas[j]); }
        for (int q = tid; q < na * 4; q += 256) red[q] = 0.0;
    }
    for (int64_t it = 0; it < ntiles; ++it) {
        const int64_t t0 = base + it * FIT_TILE;
        const bool fit = fit_stage<T, true>(a, s, e, t0, xs, ts);  // (its first barrier also covers the tables above)
        const double yt = xs[(size_t)kt * ts + tid];
        if constexpr (KT > 0) {
            double x[KT], zz[KT], zc[KT];
#pragma unroll
            for (int i = 0; i < KT; ++i) x[i] = xs[i * ts + tid];
#pragma unroll
            for (int m = 0; m < KT; ++m) {
                double z = 0.0;
#pragma unroll
                for (int i = 0; i < KT; ++i) z = fma(Vs[i * KT + m], x[i], z);
                zz[m] = z * z;
                zc[m] = z * cs[m];
            }
            for (int j = 0; j < na; ++j) {
                const double *d = D + j * KT;
                double h = 0.0, f = 0.0;
#pragma unroll
                for (int m = 0; m < KT; ++m) { const double dm = d[m]; h = fma(zz[m], dm, h); f = fma(zc[m], dm, f); }
                const double om = 1.0 - h, r = (yt - f) / om;
                const double term = !fit ? 0.0 : (om >= 1e-10 ? r * r : fit_nan());
                const double v = wave_sum_row3(term);
                if (lane == 63) red[j * 4 + wv] += v;
            }
        } else {
            for (int m = 0; m < kt; ++m) {
                double z = 0.0;
                for (int i = 0; i < kt; ++i) z = fma(Vs[i * kt + m], xs[i * ts + tid], z);
                zs[m * ts + tid] = z;
            }
            for (int m = 0; m < kt; ++m) {                         // (the row's own slots: x~ is no longer needed)
                const double z = zs[m * ts + tid];
                xs[m * ts + tid] = z * cs[m];
                zs[m * ts + tid] = z * z;
            }
            for (int j = 0; j < na; ++j) {
                const double *d = D + j * kt;
                double h = 0.0, f = 0.0;
                for (int m = 0; m < kt; ++m) { const double dm = d[m]; h = fma(zs[m * ts + tid], dm, h); f = fma(xs[m * ts + tid], dm, f); }
                const double om = 1.0 - h, r = (yt - f) / om;
                const double term = !fit ? 0.0 : (om >= 1e-10 ? r * r : fit_nan());
                const double v = wave_sum_row3(term);
                if (lane == 63) red[j * 4 + wv] += v;
            }
        }
        __syncthreads();                                           // the next tile overwrites xs
    }
    __syncthreads();
    if (tid < na) a.score_part[(size_t)blockIdx.x * na + tid] = (red[tid * 4] + red[tid * 4 + 1]) + (red[tid * 4 + 2] + red[tid * 4 + 3]);
}

static size_t k10_rows_lds(int kt, int na, bool parked) {
    return sizeof(double) * ((size_t)(kt + 2) * FIT_TILE + (parked ? (size_t)kt * FIT_TILE : 0) + (size_t)kt * kt + kt + (size_t)na * kt + (size_t)na * 4);
}

template <typename T, int KT>
static int k10_rows_launch_kt(pols_ctx *ctx, const RidgeCvArgs &a) {
    const size_t lds = k10_rows_lds(a.kt, a.n_alphas, KT == 0);
    if (lds > FIT_LDS_BUDGET) return fail(POLS_ERR_UNSUPPORTED, "ridge_cv: %d columns x %d candidates exceed the LDS of a workgroup", a.kt, a.n_alphas);
    static OncePerDevice once;
    return fit_launch(ctx, &k10_rows_kernel<T, KT>, once, fit_items(a), 256, lds, FIT_LDS_BUDGET, a);
}

template <typename T>
static int k10_rows_launch_t(pols_ctx *ctx, const RidgeCvArgs &a) {
    switch (a.kt) {
#define K10_CASE(K) case K: return k10_rows_launch_kt<T, K>(ctx, a);
        K10_CASE(1) K10_CASE(2) K10_CASE(3) K10_CASE(4) K10_CASE(5) K10_CASE(6) K10_CASE(7) K10_CASE(8)
        K10_CASE(9) K10_CASE(10) K10_CASE(11) K10_CASE(12) K10_CASE(13) K10_CASE(14) K10_CASE(15) K10_CASE(16)
#undef K10_CASE
        default: return k10_rows_launch_kt<T, 0>(ctx, a);
    }
}

int k10_rows_launch(pols_ctx *ctx, int dtype, const RidgeCvArgs &a) {
    if (a.kt < 1 || a.kt > K10_KMAX) return fail(POLS_ERR_UNSUPPORTED, "ridge_cv: %d features (incl. intercept) outside 1..%d", a.kt, K10_KMAX);
    if (a.n_alphas < 1 || a.n_alphas > K10_MAX_ALPHAS) return fail(POLS_ERR_UNSUPPORTED, "ridge_cv: %d candidates outside 1..%d", a.n_alphas, K10_MAX_ALPHAS);
    if (a.n_groups == 0) return POLS_OK;
    return dtype == POLS_F32 ? k10_rows_launch_t<float>(ctx, a) : k10_rows_launch_t<double>(ctx, a);
}

// ---------------------------------------------------------------- pick
__global__ void __launch_bounds__(64) k10_pick_kernel(const RidgeCvArgs a) {
    __shared__ double Vs[K10_KMAX * K10_KMAX], ss[K10_KMAX], cs[K10_KMAX], sc_s[K10_MAX_ALPHAS];
    const int lane = threadIdx.x, kt = a.kt, na = a.n_alphas;
    const int64_t g = blockIdx.x;
    const int64_t v0 = a.seg_offs ? a.seg_first[g] : g, v1 = a.seg_offs ? a.seg_first[g + 1] : g + 1;
    const double *E = a.eig + (size_t)g * k10_eig_stride(kt);
    for (int q = lane; q < kt * kt; q += 64) Vs[q] = E[q];
    if (lane < kt) { ss[lane] = E[kt * kt + lane]; cs[lane] = E[kt * kt + kt + lane]; }
    const double n = E[kt * kt + 2 * kt];
    __syncthreads();
    const double aj = lane < na ? a.alphas[lane] : 0.0;
    double sc = fit_nan();
    if (lane < na && n > 0.0) {
        double tot = 0.0;
        for (int64_t it = v0; it < v1; ++it) tot += a.score_part[(size_t)it * na + lane];
        double smin = ss[0], smax = ss[0];
        for (int m = 1; m < kt; ++m) { smin = fmin(smin, ss[m]); smax = fmax(smax, ss[m]); }
        const bool factors = smin + aj > 16.0 * (double)kt * FIT_EPS * (smax + aj);   // (false for NaN too)
        if (factors) sc = tot / n;
    }
    if (lane < na) {
        sc_s[lane] = sc;
        if (a.cv_scores) a.cv_scores[(size_t)g * na + lane] = sc;
    }
    __syncthreads();
    int best = -1;
    double bv = 0.0;
    for (int j = 0; j < na; ++j) { const double v = sc_s[j]; if (v == v && (best < 0 || v < bv)) { best = j; bv = v; } }
    auto put = [&](void *p, size_t at, double v) {
        if (a.f32) static_cast<float *>(p)[at] = (float)v; else static_cast<double *>(p)[at] = v;
    };
    if (lane < na && (a.coef_path || lane == best)) {
        for (int i = 0; i < kt; ++i) {
            double bi = 0.0;
            for (int m = 0; m < kt; ++m) bi = fma(Vs[i * kt + m], cs[m] / (ss[m] + aj), bi);
            if (!(sc == sc)) bi = fit_nan();
            if (a.coef_path) put(a.coef_path, ((size_t)g * na + lane) * kt + i, bi);
            if (lane == best) {
                if (a.coef) put(a.coef, (size_t)g * kt + i, bi);
                a.coef64[(size_t)g * kt + i] = bi;
            }
        }
    }
    if (lane == 0) {
        if (best < 0) {
            const double fillv = n > 0.0 ? fit_nan() : 0.0;        // no rows: zeros, as the existing entry; nothing usable: NaN
            for (int i = 0; i < kt; ++i) {
                if (a.coef) put(a.coef, (size_t)g * kt + i, fillv);
                a.coef64[(size_t)g * kt + i] = fillv;
            }
        }
        if (a.alpha) a.alpha[g] = best >= 0 ? a.alphas[best] : fit_nan();
        if (a.alpha_index) a.alpha_index[g] = best;
        if (a.score) a.score[g] = best >= 0 ? bv : fit_nan();
        if (a.status) a.status[g] = best >= 0 ? POLS_GROUP_OK : (n > 0.0 ? POLS_GROUP_FALLBACK : POLS_GROUP_EMPTY);
    }
}

int k10_pick_launch(pols_ctx *ctx, const RidgeCvArgs &a) {
    if (a.n_groups == 0) return POLS_OK;
    hipLaunchKernelGGL(k10_pick_kernel, dim3((unsigned)a.n_groups), dim3(64), 0, ctx->stream, a);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

// ---------------------------------------------------------------- predict
template <typename T>
__global__ void __launch_bounds__(256) k10_predict_kernel(const RidgeCvArgs a) {
    const int ku = a.k_user, kt = a.kt;
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    if (e <= s) return;
    const double *cg = a.coef64 + (size_t)g * kt;
    const T *wp = static_cast<const T *>(a.w);
    T *const out[3] = {static_cast<T *>(a.pred), static_cast<T *>(a.resid), nullptr};
    fit_predict_rows<T>(a, s, e, base, cg, kt > ku ? cg[ku] : 0.0, (const T *)nullptr, out,
                        [&](double q, const double yv, const int64_t r, const bool in, const bool fit, double (&o)[3]) {
                            if (wp) { const double sw = sqrt((double)(in ? wp[r] : T(1))); q = (q * sw) * (1.0 / sw); }
                            if (!fit) q = fit_nan();
                            o[0] = q;
                            o[1] = yv - q;
                        });
}

int k10_predict_launch(pols_ctx *ctx, int dtype, const RidgeCvArgs &a) {
    if (a.n_groups == 0 || a.n_rows == 0 || (!a.pred && !a.resid)) return POLS_OK;
    const int64_t n_items = fit_items(a);
    if (dtype == POLS_F32) hipLaunchKernelGGL(k10_predict_kernel<float>, dim3((unsigned)n_items), dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(k10_predict_kernel<double>, dim3((unsigned)n_items), dim3(256), 0, ctx->stream, a);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

}  // namespace pols
