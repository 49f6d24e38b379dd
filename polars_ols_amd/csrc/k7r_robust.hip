// k7r_robust.hip -- K7r: robust standard errors of mode="statistics" (pols_least_squares_statistics_robust).
//
// Per group, on the rows the null policy leaves, scaled by sqrt(w), the ones column last (as K7):
//   A = X'X + lambda I,  b = A^-1 X'y (K7's side-car coefficients),  e_i = y_i - x_i'b,  h_i = x_i' A^-1 x_i,
//   u_i = c_i e_i x_i  with c_i = 1 (HC0, HC1, HAC), (1 - h_i)^-1/2 (HC2), (1 - h_i)^-1 (HC3),
//   S = sum_i u_i u_i'  [+ sum_{l=1..L} (1 - l / (L + 1)) sum_i (u_i u_{i-l}' + u_{i-l} u_i')  for HAC, L = min(maxlags, n - 1)],
//   V = A^-1 S A^-1 (x n / df for HC1),  se_j = sqrt(V_jj),  t_j = b_j / se_j,  p_j two-sided Student-t with K7's df.
// Three launches:
//   prepare  one wave per group: K7's Cholesky solve (k7_small_solve), then the whole A^-1 = M'M (M = L^-1), b, trace(A^-1), ok;
//   meat     one 256-thread workgroup per segment of a long group (ensure_segments) or per group: tiles of rows staged as U in LDS
//            behind a halo of the previous tile's last L rows; w_i = u_i / 2 + sum_l w_l u_{i-l} column by column from LDS (L k per row,
//            exact inside the tile -- no long-range prefix sums), Q += U'W, so that S = Q + Q' = U'U + T + T' with T = U'(W - U/2):
//            k^2 + L k FMAs per row.  A segment's first L rows take their lag partners from the rows just before it in its group;
//   finish   one workgroup per group: Q summed over the group's segments in a fixed order (the same sums whatever ran first, as
//            k7_finish_kernel), the sandwich's diagonal, the HC1 factor, se / t / p.
// Everything is f64, like K7.
#include "k7r_robust.hpp"

namespace pols {

template <typename T>
__global__ void __launch_bounds__(64) k7r_prepare_kernel(const RobustArgs r) {
    __shared__ double L[K7_KMAX * K7_KMAX], M[K7_KMAX * K7_KMAX];
    __shared__ double rinv[K7_KMAX], bvec[K7_KMAX], tvec[K7_KMAX], binv[K7_KMAX], cdis[K7_KMAX], dg[K7_KMAX];
    __shared__ int okflag;
    const StatsArgs &a = r.s;
    const int64_t g = blockIdx.x;
    const int lane = threadIdx.x, kt = a.kt, E = kt * kt;
    k7_small_solve<T>(a, g, lane, L, M, rinv, bvec, tvec, binv, cdis, dg, &okflag);
    __syncthreads();
    double *P = r.prep + (size_t)g * k7r_prep_stride(kt);
    for (int q = lane; q < E; q += 64) {                           // (A^-1)_ij = sum_{p >= max(i, j)} M_pi M_pj
        const int i = q / kt, j = q - i * kt;
        double acc = 0.0;
        for (int p = i > j ? i : j; p < kt; ++p) acc += M[p * kt + i] * M[p * kt + j];
        P[q] = acc;
    }
    if (lane < kt) P[E + lane] = binv[lane];
    if (lane == 0) {
        double trace = 0.0;
        for (int j = 0; j < kt; ++j) trace += dg[j];               // K7's order: the same df
        P[E + kt] = trace;
        P[E + kt + 1] = (double)okflag;
    }
}

// u of row `row` into urow[0..kt): the scaled regressors times c e.  LEV (HC2 / HC3): the leverage from A^-1 in LDS; a row with
// 1 - h < 1e-10 sets *bad (the group's se / t / p become NaN) and contributes nothing.
template <typename T, bool LEV>
__device__ __forceinline__ void k7r_row(const StatsArgs &a, int64_t row, double *urow, const double *Ainv, const double *binv, bool hc3,
                                        bool *bad) {
    const int kt = a.kt, ku = a.k_user;
    const T *wp = static_cast<const T *>(a.w);
    const double sw = wp ? sqrt((double)wp[row]) : 1.0;
    double p = 0.0;
    for (int j = 0; j < kt; ++j) {
        const double x = ((j < ku) ? (double)static_cast<const T *>(a.x[j])[row] : 1.0) * sw;
        urow[j] = x;
        p = fma(x, binv[j], p);
    }
    double f = (double)static_cast<const T *>(a.y)[row] * sw - p;
    if (LEV) {
        double h = 0.0;
        for (int i = 0; i < kt; ++i) {
            double t = 0.0;
            for (int j = 0; j < kt; ++j) t = fma(Ainv[i * kt + j], urow[j], t);
            h = fma(urow[i], t, h);
        }
        const double om = 1.0 - h;
        if (!(om >= 1e-10)) { *bad = true; f = 0.0; }
        else f = hc3 ? f / om : f / sqrt(om);
    }
    for (int j = 0; j < kt; ++j) urow[j] *= f;
}

// Slots of the U'W accumulation: E = kt^2 entries, P = max(1, 256 / E) row-parts of each (entry e of part p is slot p E + e), so
// that small k still keeps every thread busy; up to ceil(961 / 256) = 4 slots per thread at 31 columns.
constexpr int K7R_SLOTS = (K7_KMAX * K7_KMAX + 255) / 256;

template <typename T, bool LEV>
__global__ void __launch_bounds__(256) k7r_meat_kernel(const RobustArgs r) {
    extern __shared__ double lds[];
    __shared__ int badflag;
    const StatsArgs &a = r.s;
    const int tid = threadIdx.x, kt = a.kt, E = kt * kt, TR = r.tile, H = r.maxlags;
    const int64_t sgi = blockIdx.x, g = a.seg_offs ? (int64_t)a.seg_map[sgi] : sgi;
    const int64_t gs = a.offs[g], ge = a.offs[g + 1];
    const int64_t s = a.seg_offs ? a.seg_offs[sgi] : gs, e = a.seg_offs ? a.seg_offs[sgi + 1] : ge;
    const int Lg = (int)std::min<int64_t>(H, std::max<int64_t>(0, ge - gs - 1));   // L = min(maxlags, n - 1)
    const bool hc3 = r.cov_type == POLS_COV_HC3;

    // LDS: [A^-1 (LEV)] [b] [U: H + TR rows] [W: TR rows] [slot partials: max(256, E)]
    double *Ainv = lds;
    double *binv = Ainv + (LEV ? E : 0);
    double *U = binv + kt;
    double *W = U + (size_t)(H + TR) * kt;
    double *red = W + (size_t)TR * kt;
    const double *P = r.prep + (size_t)g * k7r_prep_stride(kt);
    if (LEV)
        for (int q = tid; q < E; q += 256) Ainv[q] = P[q];
    if (tid < kt) binv[tid] = P[E + tid];
    if (tid == 0) badflag = 0;
    // the halo: zeros, then the u of the (at most L) rows of the group just before the segment
    const int hn = (int)std::min<int64_t>(Lg, s - gs);
    for (int q = tid; q < (H - hn) * kt; q += 256) U[q] = 0.0;
    __syncthreads();
    bool bad = false;
    for (int t = tid; t < hn; t += 256) k7r_row<T, LEV>(a, s - hn + t, U + (size_t)(H - hn + t) * kt, Ainv, binv, hc3, &bad);

    const int Pp = E <= 256 ? 256 / E : 1, nslot = Pp * E;
    int ea[K7R_SLOTS], eb[K7R_SLOTS];
    double acc[K7R_SLOTS];
#pragma unroll
    for (int k = 0; k < K7R_SLOTS; ++k) {
        const int slot = tid + 256 * k, q = slot % E;
        ea[k] = q / kt; eb[k] = q - (q / kt) * kt;
        acc[k] = 0.0;
    }
    const int ns = tid < nslot ? (nslot - tid + 255) / 256 : 0;
    const int part = ns == 0 ? TR : (Pp > 1 ? tid / E : 0);     // (a thread without slots skips the row loop)
    const double invL = 1.0 / (double)(Lg + 1);

    for (int64_t tb = s; tb < e; tb += TR) {
        const int nr = (int)std::min<int64_t>(TR, e - tb);
        for (int t = tid; t < TR; t += 256) {
            double *urow = U + (size_t)(H + t) * kt;
            if (t < nr) k7r_row<T, LEV>(a, tb + t, urow, Ainv, binv, hc3, &bad);
            else for (int j = 0; j < kt; ++j) urow[j] = 0.0;
        }
        __syncthreads();
        for (int q = tid; q < nr * kt; q += 256) {                 // w_i = u_i / 2 + sum_l (1 - l / (L + 1)) u_{i-l}
            const double *col = U + (size_t)H * kt + q;
            double v = 0.5 * col[0];
            for (int l = 1; l <= Lg; ++l) v = fma((double)(Lg + 1 - l) * invL, col[-(int64_t)l * kt], v);
            W[q] = v;
        }
        __syncthreads();
        for (int i = part; i < nr; i += Pp) {                      // Q += U'W
            const double *ui = U + (size_t)(H + i) * kt, *wi = W + (size_t)i * kt;
#pragma unroll
            for (int k = 0; k < K7R_SLOTS; ++k)
                if (k < ns) acc[k] = fma(ui[ea[k]], wi[eb[k]], acc[k]);
        }
        if (H > 0 && tb + TR < e) {                                // the tile's last H rows become the next tile's halo
            for (int c0 = 0; c0 < H; c0 += TR) {                   // (chunks of TR rows: a chunk's source is never an earlier chunk's target)
                __syncthreads();
                const int c1 = std::min(H, c0 + TR);
                for (int q = c0 * kt + tid; q < c1 * kt; q += 256) U[q] = U[q + (size_t)TR * kt];
            }
        }
        __syncthreads();
    }
    if (bad) badflag = 1;
#pragma unroll
    for (int k = 0; k < K7R_SLOTS; ++k)
        if (k < ns) red[tid + 256 * k] = acc[k];
    __syncthreads();
    double *out = r.part + (size_t)sgi * k7r_part_stride(kt);
    for (int q = tid; q < E; q += 256) {                           // the row-parts in a fixed order
        double v = 0.0;
        for (int p = 0; p < Pp; ++p) v += red[p * E + q];
        out[q] = v;
    }
    if (tid == 0) out[E] = (double)badflag;
}

// one 256-thread workgroup per group: a group cut into a thousand segments has a thousand partials per entry -- a wave summing them
// one after the other waits on every load, so slot (entry, part) sums every Pp-th segment with four independent accumulators
// (coalesced: the entries of a segment are adjacent), and the parts meet in a fixed order: the same sums whatever ran first
template <typename T>
__global__ void __launch_bounds__(256) k7r_finish_kernel(const RobustArgs r) {
    __shared__ double S[K7_KMAX * K7_KMAX], red[K7R_SLOTS * 256];
    __shared__ int anybad;
    const StatsArgs &a = r.s;
    const int64_t g = blockIdx.x;
    const int lane = threadIdx.x, kt = a.kt, E = kt * kt;
    const int64_t n = a.offs[g + 1] - a.offs[g];
    const int64_t v0 = a.seg_offs ? a.seg_first[g] : g, v1 = a.seg_offs ? a.seg_first[g + 1] : g + 1;
    const size_t ps = k7r_part_stride(kt);
    const int Pp = E <= 256 ? 256 / E : 1, nslot = Pp * E;
    for (int slot = lane; slot < nslot; slot += 256) {
        const int q = slot % E, p = slot / E;
        double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
        int64_t v = v0 + p;
        for (; v + 3 * Pp < v1; v += 4 * Pp) {
            c0 += r.part[(size_t)v * ps + q];
            c1 += r.part[(size_t)(v + Pp) * ps + q];
            c2 += r.part[(size_t)(v + 2 * Pp) * ps + q];
            c3 += r.part[(size_t)(v + 3 * Pp) * ps + q];
        }
        for (; v < v1; v += Pp) c0 += r.part[(size_t)v * ps + q];
        red[slot] = (c0 + c1) + (c2 + c3);
    }
    if (lane == 0) {
        int b = 0;
        for (int64_t v = v0; v < v1; ++v) b |= r.part[(size_t)v * ps + E] != 0.0;
        anybad = b;
    }
    __syncthreads();
    for (int q = lane; q < E; q += 256) {
        double acc = 0.0;
        for (int p = 0; p < Pp; ++p) acc += red[p * E + q];
        S[q] = acc;
    }
    __syncthreads();
    const double *P = r.prep + (size_t)g * k7r_prep_stride(kt);
    const double *Ainv = P;
    const double nn = (double)n, trace = P[E + kt];
    const double df = (a.lambda > 0.0) ? nn - trace : nn - (double)kt;          // K7's df
    const bool ok = P[E + kt + 1] != 0.0;
    if (lane < kt) {
        const int j = lane;
        double vjj = 0.0;                                          // (A^-1 (Q + Q') A^-1)_jj
        for (int i = 0; i < kt; ++i) {
            double t = 0.0;
            for (int m = 0; m < kt; ++m) t = fma(S[i * kt + m] + S[m * kt + i], Ainv[m * kt + j], t);
            vjj = fma(Ainv[j * kt + i], t, vjj);
        }
        if (r.cov_type == POLS_COV_HC1) vjj *= nn / df;
        const double nanv = __longlong_as_double(0x7ff8000000000000LL);
        double se = nanv, tv = nanv, pv = nanv;
        if (ok && df > 0.0 && !anybad) {
            se = sqrt(vjj);
            tv = P[E + j] / se;
            pv = (tv != tv) ? nanv : k7_betai(0.5 * df, 0.5, df / (df + tv * tv));
        }
        if (a.se) a.se[g * kt + j] = se;
        if (a.tv) a.tv[g * kt + j] = tv;
        if (a.pv) a.pv[g * kt + j] = pv;
    }
}

constexpr size_t K7R_LDS_BUDGET = 160 * 1024 - 256;   // dynamic LDS of the meat kernel (its static word and some slack aside)

static size_t k7r_lds_bytes(int kt, int H, int TR, bool lev) {
    const size_t E = (size_t)kt * kt;
    return sizeof(double) * ((lev ? E : 0) + kt + (size_t)(H + TR) * kt + (size_t)TR * kt + std::max<size_t>(256, E));
}

template <typename T, bool LEV>
static int k7r_launch_t(pols_ctx *ctx, const RobustArgs &r0) {
    RobustArgs r = r0;
    const int kt = r.s.kt, H = r.maxlags;
    int TR = 256;                                                  // the widest case (31 columns, L = 255) takes 128-row tiles
    while (TR > 64 && k7r_lds_bytes(kt, H, TR, LEV) > K7R_LDS_BUDGET) TR /= 2;
    const size_t lds = k7r_lds_bytes(kt, H, TR, LEV);
    if (lds > K7R_LDS_BUDGET) return fail(POLS_ERR_UNSUPPORTED, "robust statistics: %d columns with %d lags exceed the LDS of a workgroup", kt, H);
    r.tile = TR;
    static OncePerDevice attr_once;
    if (attr_once.needed(ctx->device))
        POLS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k7r_meat_kernel<T, LEV>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)K7R_LDS_BUDGET));   // (static + dynamic LDS must stay within the 160 KiB of a workgroup)
    const int64_t n_items = r.s.seg_offs ? r.s.n_seg : r.s.n_groups;
    hipLaunchKernelGGL(k7r_prepare_kernel<T>, dim3((unsigned)r.s.n_groups), dim3(64), 0, ctx->stream, r);
    hipLaunchKernelGGL((k7r_meat_kernel<T, LEV>), dim3((unsigned)n_items), dim3(256), lds, ctx->stream, r);
    hipLaunchKernelGGL(k7r_finish_kernel<T>, dim3((unsigned)r.s.n_groups), dim3(256), 0, ctx->stream, r);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

int k7r_prepare_launch(pols_ctx *ctx, int dtype, const RobustArgs &r) {
    if (r.s.kt > K7_KMAX) return fail(POLS_ERR_UNSUPPORTED, "robust statistics: %d features (incl. intercept) > %d", r.s.kt, K7_KMAX);
    if (r.s.n_groups == 0) return POLS_OK;
    if (dtype == POLS_F32) hipLaunchKernelGGL(k7r_prepare_kernel<float>, dim3((unsigned)r.s.n_groups), dim3(64), 0, ctx->stream, r);
    else hipLaunchKernelGGL(k7r_prepare_kernel<double>, dim3((unsigned)r.s.n_groups), dim3(64), 0, ctx->stream, r);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

int k7r_robust_launch(pols_ctx *ctx, int dtype, const RobustArgs &r) {
    if (r.s.kt > K7_KMAX) return fail(POLS_ERR_UNSUPPORTED, "robust statistics: %d features (incl. intercept) > %d", r.s.kt, K7_KMAX);
    if (r.maxlags < 0 || r.maxlags > K7R_MAXLAGS) return fail(POLS_ERR_UNSUPPORTED, "robust statistics: maxlags %d outside 0..%d", r.maxlags, K7R_MAXLAGS);
    if (r.s.n_groups == 0) return POLS_OK;
    const bool lev = r.cov_type == POLS_COV_HC2 || r.cov_type == POLS_COV_HC3;
    if (dtype == POLS_F32) return lev ? k7r_launch_t<float, true>(ctx, r) : k7r_launch_t<float, false>(ctx, r);
    return lev ? k7r_launch_t<double, true>(ctx, r) : k7r_launch_t<double, false>(ctx, r);
}

}  // namespace pols
