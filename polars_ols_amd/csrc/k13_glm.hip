// k13_glm.hip -- K13: logistic / Poisson generalised linear model per group by iteratively reweighted least squares (pols_glm).
//
// Per group g, on the rows F_g that pols_least_squares fits (null policy, a null weight acting as 1e-24, a null offset counting as a
// null feature, ones column last), everything f64 on the inputs' values, with prior weights w_i and offsets o_i:
//   start  mu0 from y (binomial (y + 0.5) / 2, Poisson y + 0.1), eta0 = g(mu0), D0 = D(mu0)
//   update W_i = w_i d(mu_i),  z_i = eta_i - o_i + (y_i - mu_i) / d(mu_i),  b <- (sum W_i x_i x_i')^-1 sum W_i x_i z_i  by Cholesky (a
//          pivot fails when d^2 <= 16 kt eps A_jj),  eta_i = x_i'b + o_i,  mu_i = g^-1(eta_i) clipped,  D = 2 sum w_i u(y_i, mu_i)
//   stop   |D_new - D| <= tol (|D_new| + 0.1), or after max_iter updates (POLS_GROUP_NOT_CONVERGED)
// The edge rules are the header's (include/pols_mi355x.h).  No floating-point atomics, every sum in a fixed order: two runs of one
// form are bit-identical.
//
// Two forms, one routing per group by its length (as K11 routes):
//   resident  ONE 256-thread workgroup per group, one launch.  The group's columns x, y, w, o are staged ONCE into an LDS tile IN THE
//             BATCH DTYPE (16-byte streaming loads on the columns' 16-byte grid, null policy applied; y of a row outside the fit is
//             NaN -- that is the fit flag) and converted on use; per row the iteration keeps W and z in f64 and nothing else.  Bytes
//             per row: elem x (k_user + 1 + [w] + [o]) + 16 against K11's 8 x (kt + 2): 1 000 rows x 8 f32 columns take 57 KB, two
//             workgroups per CU (k13_resident_lds).  No static LDS: it would sit in front of the dynamic region and cost the second
//             workgroup.  The tile's column stride is odd, so the lanes of a wave -- different columns, the same row -- hit
//             different banks in the Gram pass.
//             row pass   one thread per row of a tile: eta as one FMA chain over the columns in order, mu, the deviance term (summed
//                        per thread over its tiles, then over the wave by DPP, then waves ((0 + 1) + (2 + 3))), W and z
//             gram       [X | z]' diag(W) [X | z] with K10's assignment of the (kt + 1)(kt + 2) / 2 entries to threads (tri_spread;
//                        row partitions summed in partition order); the ones column is the constant 1
//             solve      wave 0: the family's Cholesky solve (fit_solve.inl); the standard errors come from the factor left in LDS
//   split     every other group, of any length: the segments of ensure_segments, two launches per iteration --
//             segment pass  a workgroup per segment: the row pass from the group's current f64 coefficients (the start values in the
//                        first pass) and the Gram partials of its 256-row tiles, written per segment
//             group pass    a wave per group: the segments' partials summed in segment order, the stop test on the deviance, the
//                        Cholesky solve, the next coefficients and their standard errors into the group's state, status
//             The segments and the wave of a finished group exit at once.  The host launches the pair until a device counter of the
//             groups that still iterate reads zero.
//   predict   pred = mu, resid = y - mu, linpred = eta over every row of the frame as pols_least_squares leaves them: features and
//             offsets zero-filled under every policy but "ignore", "drop" masks the rows outside the fit.  The walk is
//             fit_predict_rows (fit_tile.inl): sums in f64 and rounds once.
#include "k13_glm.hpp"
#include "fit_launch.hpp"
#include "fit_solve.inl"

namespace pols {

constexpr size_t K13_LDS_HALF = 80 * 1024 - 256;   // a request up to here leaves room for a second workgroup on the CU

// doubles in front of the tile: W and z per row, Gram partials (256), the packed Gram matrix, the Cholesky work and the inverse of
// its factor (kt x (kt + 1) each), right-hand side, Gram diagonal, coefficients, four wave sums, two integer pairs
__host__ __device__ inline size_t k13_small(int kt) {
    const size_t ne = (size_t)(kt + 1) * (kt + 2) / 2;
    return 256 + ((ne + 1) & ~(size_t)1) + 2 * (size_t)kt * (kt + 1) + 3 * (size_t)kt + 4 + 2;
}

size_t k13_resident_lds(int kt, int cols, size_t elem, int tiles) {
    const size_t rows = (size_t)tiles * FIT_TILE;
    return (sizeof(double) * (2 * rows + k13_small(kt)) + elem * (size_t)cols * (rows + 1) + 15) & ~(size_t)15;
}

int k13_resident_tiles(int kt, int cols, size_t elem, int per_cu) {
    const size_t budget = per_cu >= 2 ? K13_LDS_HALF : FIT_LDS_BUDGET;
    int nt = 0;
    while (k13_resident_lds(kt, cols, elem, nt + 1) <= budget) ++nt;
    return nt;
}

__device__ __forceinline__ bool k13_finite(const double v) { return fabs(v) <= FIT_DBL_MAX; }

// mu = g^-1(eta) clipped to the family's open range, and d(mu); a NaN stays a NaN
__device__ __forceinline__ void k13_mean(const int family, const double eta, double &mu, double &d) {
    if (family == POLS_GLM_BINOMIAL) {
        double m = 1.0 / (1.0 + exp(-eta));
        m = m < FIT_EPS ? FIT_EPS : m;
        m = m > 1.0 - FIT_EPS ? 1.0 - FIT_EPS : m;
        mu = m; d = m * (1.0 - m);
    } else {
        double m = exp(eta);
        m = m < FIT_EPS ? FIT_EPS : m;
        mu = m; d = m;
    }
}
__device__ __forceinline__ double k13_variance(const int family, const double mu) { return family == POLS_GLM_BINOMIAL ? mu * (1.0 - mu) : mu; }
__device__ __forceinline__ void k13_start(const int family, const double y, double &mu, double &eta) {
    if (family == POLS_GLM_BINOMIAL) { mu = (y + 0.5) * 0.5; eta = log(mu / (1.0 - mu)); }
    else { mu = y + 0.1; eta = log(mu); }
}
// u(y, mu), 0 log 0 = 0
__device__ __forceinline__ double k13_unit_deviance(const int family, const double y, const double mu) {
    const double t = y > 0.0 ? y * log(y / mu) : 0.0;
    if (family == POLS_GLM_BINOMIAL) return t + (y < 1.0 ? (1.0 - y) * log((1.0 - y) / (1.0 - mu)) : 0.0);
    return t - (y - mu);
}
__device__ __forceinline__ bool k13_in_domain(const int family, const double y) {
    return family == POLS_GLM_BINOMIAL ? (y >= 0.0 && y <= 1.0) : y >= 0.0;   // (false for a NaN)
}
// a fitted row at (eta, mu, d): its working weight, working response and deviance term
__device__ __forceinline__ void k13_work(const int family, const double y, const double w, const double o, const double eta, const double mu,
                                         const double d, double &W, double &z, double &dev) {
    W = w * d;
    z = eta - o + (y - mu) / d;
    dev = w * k13_unit_deviance(family, y, mu);
}

// rows [t0, t0 + 256) of the item [s, e) into xt (column stride ts, batch dtype): features 0 .. ku - 1 (nulls zero-filled unless
// "ignore"), y at ku (NaN for a row outside the fit), then w and o where the batch has them.  Returns whether this thread's row
// (t0 + tid) is a fitted row and, if so, its y, w, o; bad: a fitted row whose y is outside the family's domain.  Ends on a barrier.
template <typename T, bool STREAM>
__device__ __forceinline__ bool k13_stage(const GlmArgs &a, const int64_t s, const int64_t e, const int64_t t0, T *xt, const int ts,
                                          double &yv, double &wv, double &ov, bool &bad) {
    using V = typename Vec16<T>::type;
    constexpr int VEC = Vec16<T>::N, CH = FIT_TILE / VEC;
    const int tid = threadIdx.x, ku = a.k_user;
    const int wc = ku + 1, oc = ku + 1 + (a.w ? 1 : 0), nld = oc + (a.o ? 1 : 0);
    for (int p = tid; p < nld * CH; p += 256) {                    // (fit_stage's load loop, in the batch dtype and with the offset column)
        const int q = __builtin_amdgcn_readfirstlane(p / CH), ch = p - q * CH;     // (CH is 64 or 128: a wave stays inside one column)
        const int64_t row0 = t0 + (int64_t)ch * VEC;
        if (row0 >= e) continue;
        const void *col = q == ku ? a.y : ((q == wc && a.w) ? a.w : a.o);          // (a run-time index into the kernel arguments would put them in scratch)
#pragma unroll
        for (int j = 0; j < POLS_MAX_FEATURES; ++j) col = (j == q && j < ku) ? a.x[j] : col;
        const T *src = static_cast<const T *>(col);
        T *dst = xt + (size_t)q * ts + ch * VEC;
        if (row0 + VEC <= a.n_rows) {                              // (the columns are 16-byte aligned and row0 sits on their grid)
            const V v = STREAM ? load_stream(reinterpret_cast<const V *>(src + row0)) : *reinterpret_cast<const V *>(src + row0);
#pragma unroll
            for (int i = 0; i < VEC; ++i) dst[i] = vget<T>(v, i);
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) dst[i] = row0 + i < a.n_rows ? src[row0 + i] : T(0);
        }
    }
    __syncthreads();
    const int64_t row = t0 + tid;
    const int pol = a.null_policy;
    bool fit = row >= s && row < e;
    yv = fit ? (double)xt[(size_t)ku * ts + tid] : 0.0;
    wv = fit && a.w ? (double)xt[(size_t)wc * ts + tid] : 1.0;
    ov = fit && a.o ? (double)xt[(size_t)oc * ts + tid] : 0.0;
    if (fit && pol != POLS_NULL_IGNORE) {                          // which rows leave the fit (compute_is_valid_mask, ex.rs:201-228)
        if (a.valid && null_checks_y(pol)) fit = a.valid[row] != 0;
        if (null_checks_y(pol)) fit = fit && yv == yv;
        if (null_checks_x(pol)) {
            fit = fit && ov == ov;
            for (int c = 0; c < ku; ++c) { const T v = xt[(size_t)c * ts + tid]; fit = fit && v == v; }
        }
        if (yv != yv) yv = 0.0;                                    // handle_nulls (ex.rs:257-296)
        if (ov != ov) ov = 0.0;
    }
    for (int c = 0; c < ku; ++c) {
        T v = xt[(size_t)c * ts + tid];
        if (pol != POLS_NULL_IGNORE && v != v) v = T(0);
        xt[(size_t)c * ts + tid] = fit ? v : T(0);
    }
    if (a.o) xt[(size_t)oc * ts + tid] = fit ? (T)ov : T(0);
    bad = fit && !k13_in_domain(a.family, yv);
    xt[(size_t)ku * ts + tid] = fit ? (T)yv : (T)fit_nan();
    __syncthreads();
    return fit;
}

// tri_accumulate with the terms W x_i x_j over the rows [0, rows); column c of [X | z]: c < ku the tile's, ku < kt the ones column, kt
// the z column
template <typename T>
__device__ __forceinline__ void k13_accumulate(const TriSpread &en, double (&acc)[3], const T *xt, const int ts, const double *Wv,
                                               const double *zv, const int rows, const int ku, const int kt) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (!en.on[q]) continue;
        const int i = en.ei[q], j = en.ej[q];
        const T *ci = xt + (size_t)(i < ku ? i : 0) * ts, *cj = xt + (size_t)(j < ku ? j : 0) * ts;
        double v = acc[q];
#pragma unroll 4
        for (int r = en.part; r < rows; r += en.parts) {           // (unrolled: the LDS reads of four rows in flight)
            const double xi = i < ku ? (double)ci[r] : (i < kt ? 1.0 : zv[r]);
            const double xj = j < ku ? (double)cj[r] : (j < kt ? 1.0 : zv[r]);
            v = fma(Wv[r] * xi, xj, v);
        }
        acc[q] = v;
    }
}
// se_j = sqrt([(L L')^-1]_jj) from the factor L in the lower triangle of A: lane j builds column j of L^-1 in Li.  One wave.
__device__ __forceinline__ double k13_std_error(const double *A, double *Li, const int kt, const int lane) {
    const int LD = kt + 1;
    double ss = 0.0;
    if (lane < kt) {
        for (int i = lane; i < kt; ++i) {
            double v = i == lane ? 1.0 : 0.0;
            for (int k = lane; k < i; ++k) v -= A[i * LD + k] * Li[k * LD + lane];
            v /= A[i * LD + i];
            Li[i * LD + lane] = v;
            ss = fma(v, v, ss);
        }
    }
    return sqrt(ss);
}

__device__ __forceinline__ void k13_put_coef(const GlmArgs &a, const int64_t g, const int j, const double v) {
    a.coef64[(size_t)g * a.kt + j] = v;
    if (a.coef) { if (a.f32) static_cast<float *>(a.coef)[(size_t)g * a.kt + j] = (float)v; else static_cast<double *>(a.coef)[(size_t)g * a.kt + j] = v; }
}

// the tiles of group g, whatever its segments
template <typename T>
__device__ __forceinline__ int k13_group_tiles(const GlmArgs &a, const int64_t g) {
    return (int)min(fit_tiles<T>(a.offs[g], a.offs[g + 1]), (int64_t)0x7fffffff);
}

// ---------------------------------------------------------------- resident
template <typename T>
__global__ void __launch_bounds__(256) k13_glm_resident(const GlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, kt = a.kt, ku = a.k_user, nz = kt + 1, ne = nz * (nz + 1) / 2, LD = kt + 1;
    const int64_t g = blockIdx.x, s = a.offs[g], e = a.offs[g + 1], base = fit_base<T>(s), gt = fit_tiles<T>(s, e);
    if (gt <= a.res_from || gt > a.res_to) return;                 // the other resident launch's or the split form's group
    const int ntiles = (int)gt;
    const int ts = a.ts, R = ts - 1, fam = a.family;
    double *Wv = dyn, *zv = Wv + R, *gp = zv + R, *Gm = gp + 256;
    double *A = Gm + ((ne + 1) & ~1), *Li = A + kt * LD, *rhs = Li + kt * LD, *d0 = rhs + kt, *bc = d0 + kt, *red = bc + kt;
    int *cnt = reinterpret_cast<int *>(red + 4);                   // fitted rows, rows outside the domain, the solve's verdict
    T *xs = reinterpret_cast<T *>(red + 6);                        // (k_user + 1 + [w] + [o]) x ts
    const int wc = ku + 1, oc = ku + 1 + (a.w ? 1 : 0);
    const TriSpread en = tri_spread(kt + 1, tid);
    double acc[3] = {0.0, 0.0, 0.0};

    // ---- start: stage, count, mu0 / eta0 / D0, the first W and z
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();
    double dsum = 0.0;
    for (int it = 0; it < ntiles; ++it) {
        double yv, w, o;
        bool bad;
        const bool fit = k13_stage<T, true>(a, s, e, base + (int64_t)it * FIT_TILE, xs + (size_t)it * FIT_TILE, ts, yv, w, o, bad);
        double W = 0.0, z = 0.0;
        if (fit && !bad) {
            double mu, eta, dev;
            k13_start(fam, yv, mu, eta);
            const double d = k13_variance(fam, mu);
            k13_work(fam, yv, w, o, eta, mu, d, W, z, dev);
            dsum += dev;
        }
        Wv[it * FIT_TILE + tid] = W;
        zv[it * FIT_TILE + tid] = z;
        const unsigned long long m = __ballot(fit);
        if (lane == 0 && m) atomicAdd(&cnt[0], (int)__popcll(m));
        if (bad) cnt[1] = 1;
    }
    double D = 2.0 * fit_block_sum(dsum, red, lane, wv);
    const int n = cnt[0];
    int status = POLS_GROUP_OK, iters = 0;
    if (n == 0) status = POLS_GROUP_EMPTY;
    else if (n <= kt || cnt[1] || !k13_finite(D)) status = POLS_GROUP_FALLBACK;
    else {
        const int nr = (int)(e - base);
        for (;;) {
            k13_accumulate<T>(en, acc, xs, ts, Wv, zv, nr, ku, kt);
            tri_reduce(en, acc, gp, Gm);
            if (wv == 0) {
                const bool ok = fit_chol_solve(Gm, A, rhs, d0, kt, lane);
                if (lane == 0) cnt[2] = ok ? 1 : 0;
            }
            __syncthreads();
            if (!cnt[2]) { status = POLS_GROUP_FALLBACK; break; }
            if (tid < kt) bc[tid] = rhs[tid];
            __syncthreads();
            dsum = 0.0;
            const double icpt = kt > ku ? bc[ku] : 0.0;
            for (int it = 0; it < ntiles; ++it) {                  // the row pass: eta, mu, the deviance term, the next W and z
                const int r = it * FIT_TILE + tid;
                const double yv = (double)xs[(size_t)ku * ts + r];
                if (yv == yv) {
                    double eta = icpt;
                    for (int j = 0; j < ku; ++j) eta = fma((double)xs[(size_t)j * ts + r], bc[j], eta);
                    const double w = a.w ? (double)xs[(size_t)wc * ts + r] : 1.0, o = a.o ? (double)xs[(size_t)oc * ts + r] : 0.0;
                    eta += o;
                    double mu, d, W, z, dev;
                    k13_mean(fam, eta, mu, d);
                    k13_work(fam, yv, w, o, eta, mu, d, W, z, dev);
                    Wv[r] = W; zv[r] = z;
                    dsum += dev;
                }
            }
            const double Dn = 2.0 * fit_block_sum(dsum, red, lane, wv);
            ++iters;
            if (!k13_finite(Dn)) { status = POLS_GROUP_FALLBACK; break; }
            const bool conv = fabs(Dn - D) <= a.tol * (fabs(Dn) + 0.1);
            D = Dn;
            if (conv) break;
            if (iters >= a.max_iter) { status = POLS_GROUP_NOT_CONVERGED; break; }
        }
    }
    __syncthreads();
    // ---- outputs
    const bool fitted = status == POLS_GROUP_OK || status == POLS_GROUP_NOT_CONVERGED;
    if (tid < kt) k13_put_coef(a, g, tid, fitted ? bc[tid] : (status == POLS_GROUP_EMPTY ? 0.0 : fit_nan()));
    if (wv == 0 && a.se) {
        const double se = fitted ? k13_std_error(A, Li, kt, lane) : fit_nan();
        if (lane < kt) a.se[(size_t)g * kt + lane] = se;
    }
    if (tid == 0) {
        if (a.status) a.status[g] = status;
        if (a.deviance) a.deviance[g] = fitted ? D : fit_nan();
        if (a.n_iter) a.n_iter[g] = iters;
    }
}

template <typename T>
static int k13_resident_launch_t(pols_ctx *ctx, const GlmArgs &a) {
    const int cols = a.k_user + 1 + (a.w ? 1 : 0) + (a.o ? 1 : 0);
    const size_t lds = k13_resident_lds(a.kt, cols, sizeof(T), (a.ts - 1) / FIT_TILE);
    if (lds > FIT_LDS_BUDGET) return fail(POLS_ERR_UNSUPPORTED, "glm: %d columns x %d rows exceed the LDS of a workgroup", a.kt, a.ts);
    static OncePerDevice once;
    return fit_launch(ctx, &k13_glm_resident<T>, once, a.n_groups, 256, lds, FIT_LDS_BUDGET, a);
}

int k13_resident_launch(pols_ctx *ctx, int dtype, const GlmArgs &a) {
    if (a.kt < 1 || a.kt > K13_KMAX) return fail(POLS_ERR_UNSUPPORTED, "glm: %d features (incl. intercept) outside 1..%d", a.kt, K13_KMAX);
    if (a.n_groups == 0) return POLS_OK;
    return dtype == POLS_F32 ? k13_resident_launch_t<float>(ctx, a) : k13_resident_launch_t<double>(ctx, a);
}

// ---------------------------------------------------------------- split: the segment pass
template <typename T>
__global__ void __launch_bounds__(256) k13_glm_split(const GlmArgs a, const int first) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, kt = a.kt, ku = a.k_user, nz = kt + 1, ne = nz * (nz + 1) / 2;
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    if (k13_group_tiles<T>(a, g) <= a.res_tiles) return;           // the resident form's group
    const double *st = a.state + (size_t)g * k13_state_stride(kt);
    if (!first && st[0] == 0.0) return;                            // a finished group
    const int ts = FIT_TS, fam = a.family;
    double *Wv = dyn, *zv = Wv + FIT_TILE, *gp = zv + FIT_TILE, *bc = gp + 256, *red = bc + 32;
    int *cnt = reinterpret_cast<int *>(red + 4);
    T *xs = reinterpret_cast<T *>(red + 6);
    const TriSpread en = tri_spread(kt + 1, tid);
    double acc[3] = {0.0, 0.0, 0.0};
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    if (tid < kt) bc[tid] = first ? 0.0 : st[4 + tid];
    __syncthreads();
    const double icpt = kt > ku ? bc[ku] : 0.0;
    double dsum = 0.0;
    for (int64_t it = 0; it < ntiles; ++it) {
        const int64_t t0 = base + it * FIT_TILE;
        double yv, w, o;
        bool bad;
        const bool fit = k13_stage<T, false>(a, s, e, t0, xs, ts, yv, w, o, bad);   // (plain loads: the next iteration reads the rows again, from L2 / MALL)
        double W = 0.0, z = 0.0;
        if (fit && !bad) {
            double mu, eta, d, dev;
            if (first) {
                k13_start(fam, yv, mu, eta);
                d = k13_variance(fam, mu);
            } else {
                eta = icpt;
                for (int j = 0; j < ku; ++j) eta = fma((double)xs[(size_t)j * ts + tid], bc[j], eta);
                eta += o;
                k13_mean(fam, eta, mu, d);
            }
            k13_work(fam, yv, w, o, eta, mu, d, W, z, dev);
            dsum += dev;
        }
        Wv[tid] = W; zv[tid] = z;
        const unsigned long long m = __ballot(fit);
        if (lane == 0 && m) atomicAdd(&cnt[0], (int)__popcll(m));
        if (bad) cnt[1] = 1;
        __syncthreads();
        k13_accumulate<T>(en, acc, xs, ts, Wv, zv, (int)min((int64_t)FIT_TILE, e - t0), ku, kt);
        __syncthreads();                                           // the next tile overwrites xs
    }
    double *out = a.part + (size_t)blockIdx.x * k13_part_stride(kt);
    tri_reduce(en, acc, gp, out);
    const double dev = fit_block_sum(dsum, red, lane, wv);
    if (tid == 0) { out[ne] = dev; out[ne + 1] = (double)cnt[0]; out[ne + 2] = (double)cnt[1]; }
}

// ---------------------------------------------------------------- split: the group pass
__global__ void __launch_bounds__(64) k13_glm_split_group(const GlmArgs a, const int first) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int lane = threadIdx.x, kt = a.kt, nz = kt + 1, ne = nz * (nz + 1) / 2;
    double *Gm = dyn, *A = Gm + ne + 3, *Li = A + kt * nz, *rhs = Li + kt * nz, *d0 = rhs + kt;   // (k13_group_lds)
    const int64_t g = blockIdx.x;
    if ((a.f32 ? k13_group_tiles<float>(a, g) : k13_group_tiles<double>(a, g)) <= a.res_tiles) return;
    double *st = a.state + (size_t)g * k13_state_stride(kt);
    if (!first && st[0] == 0.0) return;
    const int64_t v0 = a.seg_offs ? a.seg_first[g] : g, v1 = a.seg_offs ? a.seg_first[g + 1] : g + 1;
    const size_t ps = k13_part_stride(kt);
    for (int en = lane; en < ne + 3; en += 64) {                   // the segments' partials in segment order
        double v = 0.0;
        for (int64_t it = v0; it < v1; ++it) v += a.part[(size_t)it * ps + en];
        Gm[en] = v;
    }
    fit_wave_sync();
    const double D = 2.0 * Gm[ne];
    int status = -1, iters = first ? 0 : (int)st[2];               // -1: the iteration goes on
    if (first) {
        const double n = Gm[ne + 1];
        if (n == 0.0) status = POLS_GROUP_EMPTY;
        else if (n <= (double)kt || Gm[ne + 2] != 0.0 || !k13_finite(D)) status = POLS_GROUP_FALLBACK;
    } else {
        if (!k13_finite(D)) status = POLS_GROUP_FALLBACK;
        else if (fabs(D - st[1]) <= a.tol * (fabs(D) + 0.1)) status = POLS_GROUP_OK;
        else if (iters >= a.max_iter) status = POLS_GROUP_NOT_CONVERGED;
    }
    if (status < 0) {
        const bool ok = fit_chol_solve(Gm, A, rhs, d0, kt, lane);
        if (!ok) status = POLS_GROUP_FALLBACK;
        else {
            fit_wave_sync();
            const double se = k13_std_error(A, Li, kt, lane);
            if (lane < kt) { st[4 + lane] = rhs[lane]; st[4 + kt + lane] = se; }
            if (lane == 0) { st[0] = 1.0; st[1] = D; st[2] = (double)(iters + 1); }
            return;
        }
    }
    // ---- finished: outputs
    const bool fitted = status == POLS_GROUP_OK || status == POLS_GROUP_NOT_CONVERGED;
    if (lane < kt) {
        k13_put_coef(a, g, lane, fitted ? st[4 + lane] : (status == POLS_GROUP_EMPTY ? 0.0 : fit_nan()));
        if (a.se) a.se[(size_t)g * kt + lane] = fitted ? st[4 + kt + lane] : fit_nan();
    }
    if (lane == 0) {
        if (a.status) a.status[g] = status;
        if (a.deviance) a.deviance[g] = fitted ? D : fit_nan();
        if (a.n_iter) a.n_iter[g] = iters;
        st[0] = 0.0;
        atomicSub(a.active, 1);
    }
}

static size_t k13_group_lds(int kt) { return sizeof(double) * ((size_t)(kt + 1) * (kt + 2) / 2 + 3 + 2 * (size_t)kt * (kt + 1) + 2 * (size_t)kt); }
static size_t k13_split_lds(int cols, size_t elem) {
    return (sizeof(double) * (3 * 256 + 32 + 4 + 2) + elem * (size_t)cols * FIT_TS + 15) & ~(size_t)15;
}

template <typename T>
static int k13_split_launch_t(pols_ctx *ctx, const GlmArgs &a, bool first) {
    const int cols = a.k_user + 1 + (a.w ? 1 : 0) + (a.o ? 1 : 0);
    static OncePerDevice once;
    const int rc = fit_launch(ctx, &k13_glm_split<T>, once, fit_items(a), 256, k13_split_lds(cols, sizeof(T)), FIT_LDS_BUDGET, a, first ? 1 : 0);
    if (rc) return rc;
    hipLaunchKernelGGL(k13_glm_split_group, dim3((unsigned)a.n_groups), dim3(64), k13_group_lds(a.kt), ctx->stream, a, first ? 1 : 0);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

int k13_split_launch(pols_ctx *ctx, int dtype, const GlmArgs &a, bool first) {
    if (a.kt < 1 || a.kt > K13_KMAX) return fail(POLS_ERR_UNSUPPORTED, "glm: %d features (incl. intercept) outside 1..%d", a.kt, K13_KMAX);
    if (a.n_groups == 0) return POLS_OK;
    return dtype == POLS_F32 ? k13_split_launch_t<float>(ctx, a, first) : k13_split_launch_t<double>(ctx, a, first);
}

// ---------------------------------------------------------------- predict
template <typename T>
__global__ void __launch_bounds__(256) k13_glm_predict(const GlmArgs a) {
    const int ku = a.k_user, kt = a.kt, fam = a.family;
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    if (e <= s) return;
    const double *cg = a.coef64 + (size_t)g * kt;
    T *const out[3] = {static_cast<T *>(a.pred), static_cast<T *>(a.resid), static_cast<T *>(a.linpred)};
    fit_predict_rows<T>(a, s, e, base, cg, kt > ku ? cg[ku] : 0.0, static_cast<const T *>(a.o), out,
                        [&](double eta, const double yv, const int64_t, const bool, const bool fit, double (&o)[3]) {
                            if (!fit) eta = fit_nan();
                            double mu, d;
                            k13_mean(fam, eta, mu, d);
                            o[0] = mu;
                            o[1] = yv - mu;
                            o[2] = eta;
                        });
}

int k13_predict_launch(pols_ctx *ctx, int dtype, const GlmArgs &a) {
    if (a.n_groups == 0 || a.n_rows == 0 || (!a.pred && !a.resid && !a.linpred)) return POLS_OK;
    const int64_t n_items = fit_items(a);
    if (dtype == POLS_F32) hipLaunchKernelGGL(k13_glm_predict<float>, dim3((unsigned)n_items), dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(k13_glm_predict<double>, dim3((unsigned)n_items), dim3(256), 0, ctx->stream, a);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

}  // namespace pols
