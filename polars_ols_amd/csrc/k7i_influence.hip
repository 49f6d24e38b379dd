// k7i_influence.hip -- K7i: per-row influence diagnostics and prediction intervals (pols_least_squares_influence).
//
// Per group g, on the rows F_g that pols_least_squares_statistics_robust fits (null policy, sqrt(w) scaling with a null weight acting as
// 1e-24, ones column last), with x~_i = sqrt(w_i) x_i, y~_i = sqrt(w_i) y_i, p = kt, A = X~'X~ + alpha I over F_g, b = A^-1 X~'y~ (K7's
// side-car coefficients), n = |F_g| and K7's df (n - p, or n - trace A^-1 when alpha > 0):
//   sigma2 (group)     sum_{i in F_g} e~_i^2 / df,  e~_i = y~_i - x~_i'b           df, t_crit (group)  t_crit: the (1 - (1 - level) / 2)
//   leverage           h_i = x~_i' A^-1 x~_i                                                           Student-t quantile at df
//   student_internal   r_i = e~_i / sqrt(sigma2 (1 - h_i))
//   student_external   t_i = r_i sqrt((df - 1) / (df - r_i^2)); NaN when df - 1 <= 0 or df - r_i^2 <= 0
//   cooks_d            r_i^2 h_i / (p (1 - h_i))                                   dffits   t_i sqrt(h_i / (1 - h_i))
//   se_mean            sqrt(sigma2 h_i / w_i)  (the standard error of x_i'b in the target's units)
//   se_obs             sqrt(sigma2 (1 + h_i) / w_i)  (statsmodels' WLS convention: var_resid = scale / weights)
//   mean_lo / hi, obs_lo / hi   x_i'b -+ t_crit se_mean,  x_i'b -+ t_crit se_obs   (x_i'b un-scaled)
// Rules: a fitted row with 1 - h_i < 1e-10 (K7r's threshold) has NaN in the four influence measures, everything else of it is written.
// A row of the group that the policy left out of F_g is a NEW OBSERVATION: leverage (the same quadratic form, not bounded by 1),
// standard errors and interval ends from its features and weight, NaN influence measures -- and NaN everywhere when a feature (after
// the policy's own fill) or its weight is null.  Under "ignore" nothing is masked: NaNs propagate arithmetically.  A group whose
// factorisation failed or whose df <= 0 has NaN in every per-row output and in sigma2 / t_crit.  Everything is computed in f64; per-row
// outputs are stored in the batch dtype.  No atomics, every sum in a fixed order: two runs are bit-identical.
//
// Launches (after K7, which leaves the side-car RSS in StatsArgs::rss, and K7r's prepare launch, which leaves A^-1, b, trace, ok):
//   group  one thread per group: sigma2 = RSS / df, t_crit by safeguarded Newton steps on K7's two-sided tail (k7_betacf);
//   rows   one 256-thread workgroup per segment of a long group (ensure_segments) or per group.  The packed upper triangle of A^-1
//          (off-diagonal entries doubled) and b sit in LDS, read at the same address by every lane (broadcast).  A lane owns VEC
//          consecutive rows on a 16-byte grid of the columns: one 16-byte streaming load per column, every load issued before the
//          first use, p (p + 1) / 2 + p FMAs per row fully unrolled for KT = 1 .. 16; 16-byte streaming stores.  The chunks on a
//          segment's edges store row by row (their neighbours belong to another workgroup); the one chunk that crosses the end of
//          the columns loads from the last whole 16 bytes and shifts in registers.  17 .. 31 columns: the lane parks its 16-byte
//          column pieces in LDS (kt x 256 x 16 bytes) and runs the triangle with run-time loops over them.
//   The row pass runs over the ORIGINAL rows: with the compaction's validity bytes (MASK) a byte tells a fitted row from a new
//   observation, so nothing is scattered back.
#include "k7i_influence.hpp"

namespace pols {

__device__ __forceinline__ double k7i_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// P(|T| > t) of Student-t with df degrees of freedom: k7_betai(df / 2, 1 / 2, df / (df + t^2)) with its log-beta term lnb =
// lgamma(a + b) - lgamma(a) - lgamma(b) (a = df / 2, b = 1 / 2) computed once per group instead of once per evaluation
__device__ inline double k7i_tail(double df, double t, double lnb) {
    const double a = 0.5 * df, b = 0.5, x = df / (df + t * t);
    if (x >= 1.0) return 1.0;
    const double bt = exp(lnb + a * log(x) + b * log1p(-x));
    if (x < (a + 1.0) / (a + b + 2.0)) return bt * k7_betacf(a, b, x) / a;
    return 1.0 - bt * k7_betacf(b, a, 1.0 - x) / b;
}

// the t with P(|T| > t) = 1 - level.  The tail falls monotonically in t and its slope is minus twice the density,
// exp(lnb - log(df) / 2 - (df + 1) / 2 log1p(t^2 / df)): Newton steps from the Cornish-Fisher expansion around the normal quantile
// (Acklam's rational approximation; a plain 1 below three degrees of freedom), kept inside the bracket the signs seen so far give --
// a step that leaves it bisects, or doubles while nothing bounds it above.  An evaluation costs up to 500 continued-fraction terms at
// millions of degrees of freedom, so the start matters: two or three evaluations there.  Stops at 1e-15 or when the steps stop
// shrinking (the noise floor of the tail itself).
__device__ inline double k7i_tcrit(double df, double level) {
    const double a = 1.0 - level;
    const double lnb = lgamma(0.5 * df + 0.5) - lgamma(0.5 * df) - lgamma(0.5);
    double t = 1.0;
    if (df >= 3.0) {
        const double q = 0.5 * a;                                  // upper-tail probability of the normal start, q <= 1/2
        double z;
        if (q < 0.02425) {
            const double u = sqrt(-2.0 * log(q));
            z = -(((((-7.784894002430293e-03 * u - 3.223964580411365e-01) * u - 2.400758277161838e+00) * u - 2.549732539343734e+00) * u +
                   4.374664141464968e+00) * u + 2.938163982698783e+00) /
                ((((7.784695709041462e-03 * u + 3.224671290700398e-01) * u + 2.445134137142996e+00) * u + 3.754408661907416e+00) * u + 1.0);
        } else {
            const double u = q - 0.5, r = u * u;
            z = -(((((-3.969683028665376e+01 * r + 2.209460984245205e+02) * r - 2.759285104469687e+02) * r + 1.383577518672690e+02) * r -
                   3.066479806614716e+01) * r + 2.506628277459239e+00) * u /
                (((((-5.447609879822406e+01 * r + 1.615858368580409e+02) * r - 1.556989798598866e+02) * r + 6.680131188771972e+01) * r -
                  1.328068155288572e+01) * r + 1.0);
        }
        const double z3 = z * z * z;
        t = z + (z3 + z) / (4.0 * df) + (5.0 * z3 * z * z + 16.0 * z3 + 3.0 * z) / (96.0 * df * df);
        if (!(t > 0.0)) t = 1.0;
    }
    double lo = 0.0, hi = -1.0, prev = 1e300;                      // hi < 0: nothing bounds the root above yet
    for (int i = 0; i < 1200; ++i) {
        const double f = k7i_tail(df, t, lnb) - a;
        if (f > 0.0) lo = t; else hi = t;
        const double dens = exp(lnb - 0.5 * log(df) - 0.5 * (df + 1.0) * log1p(t * t / df));
        double tn = t + f / (2.0 * dens);
        double step = fabs(tn - t);
        if (step <= 1e-15 * t || (step < 1e-7 * t && step >= 0.25 * prev)) {     // converged, or at the tail's own noise floor
            if (tn >= lo && (hi < 0.0 || tn <= hi)) t = tn;
            break;
        }
        if (!(tn > lo) || (hi > 0.0 && !(tn < hi))) {
            tn = hi > 0.0 ? 0.5 * (lo + hi) : 2.0 * t;
            step = fabs(tn - t);
            if (!(tn > lo) || (hi > 0.0 && !(tn < hi))) break;                  // the bracket has closed
        }
        prev = step;
        t = tn;
    }
    return t;
}

// f32 batches.  The Gram matrix of an f32 frame is accumulated in f32 pieces (k5_enet.hip, k5v_gram.hip), which leaves b = A^-1 X~'y~ with
// f32-sized errors: harmless for the per-coefficient statistics, but a row's residual y~ - x~'b is a difference, and the rows it nearly
// vanishes on keep no digits of it.  One step of iterative refinement mends that: the residual of the normal equations
// X~'(y~ - X~ b) - alpha b, summed in f64 from the columns themselves (this pass), then b += A^-1 (that) in the group stage.
// One 256-thread workgroup per segment / group; 32 statically indexed accumulators (a run-time kt guards them): no scratch.
template <typename T>
__global__ void __launch_bounds__(256) k7i_refine_kernel(const RobustArgs r) {
    __shared__ double bs[K7_KMAX + 1], red[K7_KMAX + 1][4];
    const StatsArgs &a = r.s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, kt = a.kt, ku = a.k_user;
    const int64_t sgi = blockIdx.x, g = a.seg_offs ? (int64_t)a.seg_map[sgi] : sgi;
    const int64_t s = a.seg_offs ? a.seg_offs[sgi] : a.offs[g], e = a.seg_offs ? a.seg_offs[sgi + 1] : a.offs[g + 1];
    if (tid < kt) bs[tid] = r.prep[(size_t)g * k7r_prep_stride(kt) + (size_t)kt * kt + tid];
    __syncthreads();
    const T *yp = static_cast<const T *>(a.y), *wp = static_cast<const T *>(a.w);
    double acc[K7_KMAX + 1];
#pragma unroll
    for (int j = 0; j <= K7_KMAX; ++j) acc[j] = 0.0;
    for (int64_t row = s + tid; row < e; row += 256) {
        const double sw = wp ? sqrt((double)wp[row]) : 1.0;
        double p = 0.0;
#pragma unroll
        for (int j = 0; j <= K7_KMAX; ++j)
            if (j < kt) p = fma(((j < ku) ? (double)static_cast<const T *>(a.x[j])[row] : 1.0) * sw, bs[j], p);
        const double et = (double)yp[row] * sw - p;
#pragma unroll
        for (int j = 0; j <= K7_KMAX; ++j)                          // (the row's columns again: they sit in the cache the loop above filled)
            if (j < kt) acc[j] = fma(((j < ku) ? (double)static_cast<const T *>(a.x[j])[row] : 1.0) * sw, et, acc[j]);
    }
#pragma unroll
    for (int j = 0; j <= K7_KMAX; ++j) {
        if (j < kt) {
            const double v = wave_sum_row3(acc[j]);
            if (lane == 63) red[j][wv] = v;
        }
    }
    __syncthreads();
    if (tid < kt) r.part[(size_t)sgi * kt + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

int k7i_refine_launch(pols_ctx *ctx, int dtype, const RobustArgs &r) {
    if (r.s.kt > K7_KMAX) return fail(POLS_ERR_UNSUPPORTED, "influence: %d features (incl. intercept) > %d", r.s.kt, K7_KMAX);
    if (r.s.n_groups == 0) return POLS_OK;
    const int64_t n_items = r.s.seg_offs ? r.s.n_seg : r.s.n_groups;
    if (dtype == POLS_F32) hipLaunchKernelGGL(k7i_refine_kernel<float>, dim3((unsigned)n_items), dim3(256), 0, ctx->stream, r);
    else hipLaunchKernelGGL(k7i_refine_kernel<double>, dim3((unsigned)n_items), dim3(256), 0, ctx->stream, r);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

__global__ void __launch_bounds__(256) k7i_group_kernel(const InflGroupArgs a) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.n_groups) return;
    const int kt = a.kt, E = kt * kt;
    double *P = a.prep + (size_t)g * k7r_prep_stride(kt);
    if (a.xe && P[E + kt + 1] != 0.0) {
        // b += A^-1 (X~'e~ - alpha b).  First the right-hand side, the segments' sums in segment order, parked in the group's first xe
        // row (this thread alone reads the group's rows); then the correction, which no longer reads b
        const int64_t v0 = a.seg_first ? a.seg_first[g] : g, v1 = a.seg_first ? a.seg_first[g + 1] : g + 1;
        double *rhs = a.xe + (size_t)v0 * kt;
        for (int j = 0; j < kt; ++j) {
            double gj = 0.0;
            for (int64_t v = v0; v < v1; ++v) gj += a.xe[(size_t)v * kt + j];
            rhs[j] = gj - a.lambda * P[E + j];
        }
        for (int i = 0; i < kt; ++i) {
            double d = 0.0;
            for (int j = 0; j < kt; ++j) d = fma(P[i * kt + j], rhs[j], d);
            P[E + i] += d;
        }
    }
    const double nn = (double)(a.offs[g + 1] - a.offs[g]);
    const double df = (a.lambda > 0.0) ? nn - P[E + kt] : nn - (double)kt;      // K7's df
    const bool good = P[E + kt + 1] != 0.0 && df > 0.0;
    const size_t G = (size_t)a.n_groups;
    a.grp[g] = good ? a.rss[g] / df : k7i_nan();
    a.grp[G + g] = df;
    a.grp[2 * G + g] = good ? k7i_tcrit(df, a.level) : k7i_nan();
    a.grp[3 * G + g] = good ? 1.0 : 0.0;
}

int k7i_group_launch(pols_ctx *ctx, const InflGroupArgs &a) {
    if (a.n_groups == 0) return POLS_OK;
    hipLaunchKernelGGL(k7i_group_kernel, dim3((unsigned)((a.n_groups + 255) / 256)), dim3(256), 0, ctx->stream, a);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

// ---------------------------------------------------------------- the row pass
// VEC rows of one column from row r0 (a frame shorter than one vector: guarded element loads, zeros past the end)
template <typename T>
__device__ __forceinline__ void k7i_load(const void *col, int64_t r0, bool tiny, int64_t n_rows, T (&v)[Vec16<T>::N]) {
    using V = typename Vec16<T>::type;
    constexpr int VEC = Vec16<T>::N;
    const T *p = static_cast<const T *>(col);
    if (tiny) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = r0 + e < n_rows ? p[r0 + e] : T(0);
        return;
    }
    const V ld = load_stream(reinterpret_cast<const V *>(p + r0));
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = vget<T>(ld, e);
}

// the chunk that crosses the end of the columns was loaded d rows early: element e takes what sits at e + d, zeros past the end
template <typename T>
__device__ __forceinline__ void k7i_shift(T (&v)[Vec16<T>::N], int d) {
    constexpr int VEC = Vec16<T>::N;
    T o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        T r = T(0);
#pragma unroll
        for (int f = 0; f < VEC; ++f) r = (f == e + d) ? v[f] : r;
        o[e] = r;
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = o[e];
}

__device__ __forceinline__ float4 k7i_pack(const float (&v)[4]) { return float4{v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ double2 k7i_pack(const double (&v)[2]) { return double2{v[0], v[1]}; }

// KT > 0: the unrolled build of exactly KT columns; KT == 0: run-time kt (17 .. 31), the lane's column pieces parked in dynamic LDS
template <typename T, int KT, bool HAS_W, bool MASK>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) k7i_rows_kernel(const InflArgs a) {
    using V = typename Vec16<T>::type;
    constexpr int VEC = Vec16<T>::N;
    constexpr int NPS = KT > 0 ? KT * (KT + 1) / 2 : 1, NBS = KT > 0 ? KT : 1;
    __shared__ double Ps[NPS], bs[NBS];
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int tid = threadIdx.x, kt = KT > 0 ? KT : a.kt, ku = a.k_user, np = kt * (kt + 1) / 2;
    double *P = KT > 0 ? Ps : dyn;                                 // packed rows of the upper triangle: row i starts at i kt - i (i - 1) / 2
    double *bv = KT > 0 ? bs : dyn + np;
    V *xs = reinterpret_cast<V *>(dyn + ((np + kt + 1) & ~1));     // (KT == 0) piece of column j of this lane: xs[j * 256 + tid]
    const int64_t sgi = blockIdx.x, g = a.seg_offs ? (int64_t)a.seg_map[sgi] : sgi;
    const int64_t s = a.seg_offs ? a.seg_offs[sgi] : a.offs[g], e = a.seg_offs ? a.seg_offs[sgi + 1] : a.offs[g + 1];
    {
        const double *R = a.prep + (size_t)g * k7r_prep_stride(kt);
        for (int q = tid; q < kt * kt; q += 256) {
            const int i = q / kt, j = q - i * kt;
            if (j >= i) P[i * kt - i * (i - 1) / 2 + (j - i)] = (j == i ? 1.0 : 2.0) * R[q];
        }
        if (tid < kt) bv[tid] = R[kt * kt + tid];
    }
    __syncthreads();
    const size_t G = (size_t)a.n_groups;
    const double s2 = a.grp[g], df = a.grp[G + g], tc = a.grp[2 * G + g];
    const double poison = a.grp[3 * G + g] != 0.0 ? 0.0 : k7i_nan();             // a failed group: NaN in every row
    const double dfm1 = df - 1.0, invp = 1.0 / (double)kt;
    const bool want_infl = a.out[K7I_STUDENT_INT] || a.out[K7I_STUDENT_EXT] || a.out[K7I_COOKS_D] || a.out[K7I_DFFITS];
    const bool want_se = a.out[K7I_SE_MEAN] || a.out[K7I_SE_OBS] || a.out[K7I_MEAN_LO] || a.out[K7I_MEAN_HI] || a.out[K7I_OBS_LO] ||
                         a.out[K7I_OBS_HI];
    const bool zf = MASK && a.zero_fill != 0;
    const bool tiny = a.n_rows < VEC;

    const int64_t base = s & ~(int64_t)(VEC - 1);                  // the chunk grid is the columns' 16-byte grid
    const int64_t nch = (e - base + VEC - 1) / VEC;
    for (int64_t c = tid; c < nch; c += 256) {
        const int64_t row0 = base + c * VEC;
        const bool full = row0 >= s && row0 + VEC <= e;            // no row of a neighbour in the chunk: whole 16-byte stores
        const int64_t r0 = (!tiny && row0 + VEC > a.n_rows) ? a.n_rows - VEC : row0;
        const int d = (int)(row0 - r0);
        unsigned fit = 0xffffffffu;
        if (MASK) fit = VEC == 4 ? *reinterpret_cast<const uint32_t *>(a.valid + row0) : *reinterpret_cast<const uint16_t *>(a.valid + row0);
        T yr[VEC], wr[VEC];
        k7i_load<T>(a.y, r0, tiny, a.n_rows, yr);
        if (HAS_W) k7i_load<T>(a.w, r0, tiny, a.n_rows, wr);
        double pm[VEC], qf[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) pm[v] = qf[v] = 0.0;

        if constexpr (KT > 0) {
            T xr[KT][VEC];
#pragma unroll
            for (int j = 0; j < KT; ++j) {
                if (j < ku) k7i_load<T>(a.x[j], r0, tiny, a.n_rows, xr[j]);
                else
#pragma unroll
                    for (int v = 0; v < VEC; ++v) xr[j][v] = T(1);
            }
            if (d != 0) {                                          // at most one lane per launch
                k7i_shift<T>(yr, d);
                if (HAS_W) k7i_shift<T>(wr, d);
#pragma unroll
                for (int j = 0; j < KT; ++j)
                    if (j < ku) k7i_shift<T>(xr[j], d);
            }
            // row blocks of HV rows: wide f32 chunks convert two of their four rows at a time (half the f64 copies live at once).  The
            // compiler barrier makes every block read A^-1 from LDS (same address in every lane: a broadcast) -- hoisted out of the
            // chunk loop the packed triangle alone would take p (p + 1) registers
            constexpr int HV = (sizeof(T) == 4 && KT > 8) ? 2 : VEC;
#pragma unroll
            for (int h0 = 0; h0 < VEC; h0 += HV) {
                asm volatile("" ::: "memory");
                double xd[KT][HV];
#pragma unroll
                for (int j = 0; j < KT; ++j)
#pragma unroll
                    for (int v = 0; v < HV; ++v) {
                        const T x = xr[j][h0 + v];
                        xd[j][v] = (double)((zf && x != x) ? T(0) : x);
                    }
#pragma unroll
                for (int i = 0; i < KT; ++i) {
                    double t[HV];
#pragma unroll
                    for (int v = 0; v < HV; ++v) t[v] = 0.0;
#pragma unroll
                    for (int j = i; j < KT; ++j) {
                        const double pij = P[i * KT - i * (i - 1) / 2 + (j - i)];
#pragma unroll
                        for (int v = 0; v < HV; ++v) t[v] = fma(pij, xd[j][v], t[v]);
                    }
                    const double bi = bv[i];
#pragma unroll
                    for (int v = 0; v < HV; ++v) {
                        qf[h0 + v] = fma(xd[i][v], t[v], qf[h0 + v]);
                        pm[h0 + v] = fma(xd[i][v], bi, pm[h0 + v]);
                    }
                }
            }
        } else {
            if (d != 0) {
                k7i_shift<T>(yr, d);
                if (HAS_W) k7i_shift<T>(wr, d);
            }
#pragma unroll 4
            for (int j = 0; j < kt; ++j) {
                T xr[VEC];
                if (j < ku) {
                    k7i_load<T>(a.x[j], r0, tiny, a.n_rows, xr);
                    if (d != 0) k7i_shift<T>(xr, d);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) xr[v] = (zf && xr[v] != xr[v]) ? T(0) : xr[v];
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) xr[v] = T(1);
                }
                xs[j * 256 + tid] = k7i_pack(xr);
            }
            for (int i = 0; i < kt; ++i) {
                const V xi = xs[i * 256 + tid];
                const double *Pi = P + (i * kt - i * (i - 1) / 2) - i;
                double t[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) t[v] = 0.0;
                for (int j = i; j < kt; ++j) {
                    const V xj = xs[j * 256 + tid];
                    const double pij = Pi[j];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) t[v] = fma(pij, (double)vget<T>(xj, v), t[v]);
                }
                const double bi = bv[i];
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const double x = (double)vget<T>(xi, v);
                    qf[v] = fma(x, t[v], qf[v]);
                    pm[v] = fma(x, bi, pm[v]);
                }
            }
        }

        // rows of the lane: h = w x'A^-1 x, e~ = sqrt(w) (y - x'b)
        double h[VEC], et[VEC], invw[VEC];
        bool fitted[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            fitted[v] = !MASK || ((fit >> (8 * v)) & 0xffu) != 0;
            double w = 1.0;
            if (HAS_W) {
                w = (double)wr[v];
                if (MASK && fitted[v] && w != w) w = 1e-24;        // a fitted row's null weight (least_squares.py:193)
            }
            double y = (double)yr[v];
            if (zf && fitted[v] && y != y) y = 0.0;
            h[v] = w * qf[v] + poison;
            et[v] = (y - pm[v]) * (HAS_W ? sqrt(w) : 1.0);
            invw[v] = HAS_W ? 1.0 / w : 1.0;
        }
        auto put = [&](int o, const double (&val)[VEC]) {
            T *p = static_cast<T *>(a.out[o]);
            if (!p) return;
            T tv[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) tv[v] = (T)val[v];
            if (full) store_stream(reinterpret_cast<V *>(p + row0), k7i_pack(tv));
            else {
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (row0 + v >= s && row0 + v < e) p[row0 + v] = tv[v];
            }
        };
        put(K7I_LEVERAGE, h);
        if (want_infl) {
            double ri[VEC], te[VEC], cd[VEC], dff[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const double om = 1.0 - h[v];
                const double hq = h[v] / om;
                const double r = et[v] / sqrt(s2 * om), r2 = r * r, den = df - r2;
                const double t = (dfm1 > 0.0 && den > 0.0) ? r * sqrt(dfm1 / den) : k7i_nan();
                const bool def = fitted[v] && om >= 1e-10;         // (also false for NaN)
                ri[v] = def ? r : k7i_nan();
                te[v] = def ? t : k7i_nan();
                cd[v] = def ? r2 * hq * invp : k7i_nan();
                dff[v] = def ? t * sqrt(hq) : k7i_nan();
            }
            put(K7I_STUDENT_INT, ri);
            put(K7I_STUDENT_EXT, te);
            put(K7I_COOKS_D, cd);
            put(K7I_DFFITS, dff);
        }
        if (want_se) {
            double sm[VEC], so[VEC], lo[VEC], hi[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                sm[v] = sqrt(s2 * h[v] * invw[v]);
                so[v] = sqrt(s2 * (1.0 + h[v]) * invw[v]);
            }
            put(K7I_SE_MEAN, sm);
            put(K7I_SE_OBS, so);
#pragma unroll
            for (int v = 0; v < VEC; ++v) { lo[v] = pm[v] - tc * sm[v]; hi[v] = pm[v] + tc * sm[v]; }
            put(K7I_MEAN_LO, lo);
            put(K7I_MEAN_HI, hi);
#pragma unroll
            for (int v = 0; v < VEC; ++v) { lo[v] = pm[v] - tc * so[v]; hi[v] = pm[v] + tc * so[v]; }
            put(K7I_OBS_LO, lo);
            put(K7I_OBS_HI, hi);
        }
    }
}

constexpr size_t K7I_LDS_BUDGET = 160 * 1024 - 256;

static size_t k7i_dyn_lds(int kt) {
    const size_t np = (size_t)kt * (kt + 1) / 2;
    return sizeof(double) * ((np + kt + 1) & ~(size_t)1) + (size_t)kt * 256 * 16;
}

template <typename T, int KT, bool HAS_W, bool MASK>
static int k7i_launch_one(pols_ctx *ctx, const InflArgs &a) {
    const int64_t n_items = a.seg_offs ? a.n_seg : a.n_groups;
    size_t lds = 0;
    if (KT == 0) {
        lds = k7i_dyn_lds(a.kt);
        if (lds > K7I_LDS_BUDGET) return fail(POLS_ERR_UNSUPPORTED, "influence: %d columns exceed the LDS of a workgroup", a.kt);
        static OncePerDevice attr_once;
        if (attr_once.needed(ctx->device)) {
            POLS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k7i_rows_kernel<T, KT, HAS_W, MASK>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)K7I_LDS_BUDGET));
            attr_once.done(ctx->device);
        }
    }
    hipLaunchKernelGGL((k7i_rows_kernel<T, KT, HAS_W, MASK>), dim3((unsigned)n_items), dim3(256), lds, ctx->stream, a);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

template <typename T, int KT>
static int k7i_launch_kt(pols_ctx *ctx, const InflArgs &a) {
    if (a.w) return a.valid ? k7i_launch_one<T, KT, true, true>(ctx, a) : k7i_launch_one<T, KT, true, false>(ctx, a);
    return a.valid ? k7i_launch_one<T, KT, false, true>(ctx, a) : k7i_launch_one<T, KT, false, false>(ctx, a);
}

template <typename T>
static int k7i_launch_t(pols_ctx *ctx, const InflArgs &a) {
    switch (a.kt) {
#define K7I_CASE(K) case K: return k7i_launch_kt<T, K>(ctx, a);
        K7I_CASE(1) K7I_CASE(2) K7I_CASE(3) K7I_CASE(4) K7I_CASE(5) K7I_CASE(6) K7I_CASE(7) K7I_CASE(8)
        K7I_CASE(9) K7I_CASE(10) K7I_CASE(11) K7I_CASE(12) K7I_CASE(13) K7I_CASE(14) K7I_CASE(15) K7I_CASE(16)
#undef K7I_CASE
        default: return k7i_launch_kt<T, 0>(ctx, a);
    }
}

int k7i_rows_launch(pols_ctx *ctx, int dtype, const InflArgs &a) {
    if (a.kt < 1 || a.kt > K7_KMAX) return fail(POLS_ERR_UNSUPPORTED, "influence: %d features (incl. intercept) outside 1..%d", a.kt, K7_KMAX);
    if (a.n_groups == 0 || a.n_rows == 0) return POLS_OK;
    bool any = false;
    for (int o = 0; o < K7I_NOUT; ++o) any = any || a.out[o];
    if (!any) return POLS_OK;
    return dtype == POLS_F32 ? k7i_launch_t<float>(ctx, a) : k7i_launch_t<double>(ctx, a);
}

}  // namespace pols
