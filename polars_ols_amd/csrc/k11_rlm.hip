// k11_rlm.hip -- K11: Huber / bisquare M-estimator per group by iteratively reweighted least squares (pols_rlm).
//
// Per group g, on the rows F_g that pols_least_squares fits (null policy, sqrt(w) scaling with a null weight acting as 1e-24, ones
// column last), x~_i = sqrt(w_i) x_i, y~_i = sqrt(w_i) y_i, n = |F_g|, everything f64 on the inputs' values:
//   b0 = OLS on F_g;  then per iteration  r_i = y~_i - x~_i'b,  s = median(|r_i|) / 0.6744897501960817 (exact median),
//   omega_i = psi(u_i) / u_i at u_i = |r_i| / s  (Huber: 1 | c / u;  bisquare: (1 - (u / c)^2)^2 | 0),
//   b <- (sum omega_i x~_i x~_i')^-1 sum omega_i x~_i y~_i  by Cholesky (a pivot fails when d^2 <= 16 kt eps A_jj),
//   stop when max_j |b_new - b| <= tol max(max_j |b_new|, 1e-300), or after max_iter updates, or when s collapses.
// The edge rules are the header's (include/pols_mi355x.h).  No floating-point atomics, every sum in a fixed order: two runs are
// bit-identical (the integer LDS counters of the median select do not depend on the order they are bumped in).
//
// ONE 256-thread workgroup per group runs the whole iteration in one launch, in one of two forms of the same kernel:
//   resident  the group's scaled rows [X~ | y~] and a work column (|r| or omega, sign bit set on the rows outside the fit) are staged
//             into LDS ONCE -- fit_stage: 16-byte streaming loads on the columns' 16-byte grid, null policy and sqrt(w) applied -- and
//             every iteration runs from there: the frame is read once however many iterations its groups need.  The dynamic LDS is
//             sized to the longest resident group of the launch, so short-group frames get several workgroups per CU; the column
//             stride is odd (tiles x 256 + 1), so the lanes of a wave -- different columns, the same row -- hit different banks.
//   streamed  groups whose rows do not fit: the 256-row tiles are staged again from global memory (plain loads: L2 / MALL reuse is
//             wanted) in every pass, and the work column lives in a per-row f64 buffer (Work::RlmRows).  Correct but slow; groups of
//             more than 2^22 rows are refused by the entry.
// The steps of an iteration:
//   residual  one thread per row of a tile, x~_i'b as one FMA chain over the columns in order;
//   median    radix select on the bit pattern of |r| (non-negative doubles order as unsigned integers): eight passes of a 256-bin
//             histogram in LDS (integer counters; the lanes of a wave that share a bin add once), one wave scans the bins and narrows
//             the prefix; for even n one more pass takes the smallest key above the lower middle value unless that value's own
//             multiplicity already covers the upper one;
//   weigh     omega_i over the work column, then the weighted Gram matrix [X~ | y~]' diag(omega) [X~ | y~] with K10's assignment of
//             the (kt + 1)(kt + 2) / 2 entries to threads (tri_spread's, written out; row partitions summed in partition order);
//   solve     wave 0: right-looking Cholesky in LDS (the trailing update spread over the lanes), the two substitutions, the
//             finiteness check (fit_solve.inl); every thread then evaluates the stop test on the broadcast result.
#include "k11_rlm.hpp"
#include "fit_launch.hpp"
#include "fit_solve.inl"

namespace pols {

constexpr double K11_MAD = 0.6744897501960817;     // the 0.75 quantile of the standard normal

// doubles behind the tile: Gram partials (256), the packed Gram matrix, the Cholesky work (kt x (kt + 1)), b, the previous b, the
// right-hand side, the Gram diagonal, the 256 histogram counters
__host__ __device__ inline size_t k11_extra(int kt) {
    const size_t ne = (size_t)(kt + 1) * (kt + 2) / 2;
    return 256 + ((ne + 1) & ~(size_t)1) + (size_t)kt * (kt + 1) + 4 * (size_t)kt + 128;
}
static size_t k11_lds(int kt, int ts) { return sizeof(double) * ((size_t)(kt + 2) * ts + k11_extra(kt)); }

int k11_resident_tiles(int kt) {
    int nt = 0;
    while (k11_lds(kt, (nt + 1) * FIT_TILE + 1) <= FIT_LDS_BUDGET) ++nt;
    return nt;
}

__device__ __forceinline__ unsigned long long k11_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ double k11_omega(const int norm, const double c, const double u) {
    double om;
    if (norm == POLS_RLM_HUBER) om = u <= c ? 1.0 : c / u;
    else { const double q = u / c, t = 1.0 - q * q; om = u < c ? t * t : 0.0; }
    return fabs(om);                                               // (a NaN keeps a clear sign bit: the bit marks the rows outside the fit)
}

template <typename T, bool RES>
__global__ void __launch_bounds__(256) k11_rlm_kernel(const RlmArgs a) {
    using V = typename Vec16<T>::type;
    constexpr int VEC = Vec16<T>::N;
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    __shared__ unsigned long long ymax_s, prefix_s, vmin_s;
    __shared__ int nfit_s, krem_s, cnt_s, ok_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, kt = a.kt, nz = kt + 1, ne = nz * (nz + 1) / 2, LD = kt + 1;
    const int64_t g = blockIdx.x, s = a.offs[g], e = a.offs[g + 1];
    const int64_t base = s & ~(int64_t)(VEC - 1);                  // the tile grid starts on the columns' 16-byte grid (fit_base)
    const int ntiles = e > s ? (int)((e - base + FIT_TILE - 1) / FIT_TILE) : 0;
    if (RES ? ntiles > a.res_tiles : ntiles <= a.res_tiles) return;   // the other form's group
    const int ts = a.ts;
    double *xs = dyn;                                              // (kt + 2) x ts: x~ (ones column at k_user), y~ at kt, the work column at kt + 1
    double *gp = xs + (size_t)(kt + 2) * ts;                       // 256
    double *Gm = gp + 256;                                         // ne
    double *A = Gm + ((ne + 1) & ~1);                              // kt x LD
    double *bc = A + kt * LD, *bp = bc + kt, *rhs = bp + kt, *d0 = rhs + kt;
    int *hist = reinterpret_cast<int *>(d0 + kt);                  // 256
    const size_t wc = (size_t)(kt + 1) * ts;                       // the work column

    // The thread's entries of the packed upper triangle, the accumulate and the reduce step: tri_spread, tri_accumulate and tri_reduce
    // (fit_tile.inl) written out.  This kernel keeps some 180 scalars (streamed: 330) in lanes of spare VGPRs, and with the shared
    // forms the compiler places them differently: the resident form then measures 0.2 - 0.5 % slower on 10 000 groups x 1 000 rows.
    const int parts = ne < 256 ? 256 / ne : 1;
    const int part = parts > 1 ? tid / ne : 0;
    int ei[3], ej[3];
    bool on[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int en = parts > 1 ? tid - part * ne : tid + 256 * q;
        on[q] = parts > 1 ? (q == 0 && part < parts) : en < ne;
        int i = 0, t = on[q] ? en : 0;
        while (t >= nz - i) { t -= nz - i; ++i; }
        ei[q] = i; ej[q] = i + t;
    }
    double acc[3] = {0.0, 0.0, 0.0};
    auto accumulate = [&](const double *xt, const int rows_here, const bool weighted) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (!on[q]) continue;
            const double *ci = xt + (size_t)ei[q] * ts, *cj = xt + (size_t)ej[q] * ts, *om = xt + wc;
            double v = acc[q];
            if (weighted) {
#pragma unroll 4
                for (int r = part; r < rows_here; r += parts) v = fma(om[r] * ci[r], cj[r], v);   // (unrolled: the LDS reads of four rows in flight)
            } else {
#pragma unroll 4
                for (int r = part; r < rows_here; r += parts) v = fma(ci[r], cj[r], v);
            }
            acc[q] = v;
        }
    };
    auto reduce = [&]() {                                          // acc -> Gm; ends on a barrier
        if (parts > 1) {
            if (on[0]) gp[part * ne + (tid - part * ne)] = acc[0];
            __syncthreads();
            if (tid < ne) {
                double v = 0.0;
                for (int p = 0; p < parts; ++p) v += gp[p * ne + tid];
                Gm[tid] = v;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (on[q]) Gm[tid + 256 * q] = acc[q];
        }
        acc[0] = acc[1] = acc[2] = 0.0;
        __syncthreads();
    };
    // Gm -> coefficients in rhs, ok_s; wave 0 works, ends on a barrier
    auto solve = [&]() {
        if (wv == 0) {
            const bool ok = fit_chol_solve(Gm, A, rhs, d0, kt, lane);
            if (lane == 0) ok_s = ok ? 1 : 0;
        }
        __syncthreads();
    };
    // the tile `it` with its work column in LDS; returns this thread's work value.  Streamed: stages the tile (two barriers inside).
    auto open = [&](const int it, double *&xt) -> double {
        if constexpr (RES) {
            xt = xs + (size_t)it * FIT_TILE;
            return xt[wc + tid];
        } else {
            const int64_t t0 = base + (int64_t)it * FIT_TILE, row = t0 + tid;
            xt = xs;
            fit_stage<T, false>(a, s, e, t0, xs, ts);
            return row >= s && row < e ? a.rows[row] : -1.0;
        }
    };
    auto put = [&](const int it, double *xt, const double v) {    // this thread's work value
        xt[wc + tid] = v;
        if constexpr (!RES) {
            const int64_t row = base + (int64_t)it * FIT_TILE + tid;
            if (row >= s && row < e) a.rows[row] = v;
        }
    };
    auto rows_of = [&](const int it) { return (int)min((int64_t)FIT_TILE, e - (base + (int64_t)it * FIT_TILE)); };
    auto residual = [&](const double *bb) {                        // work <- |y~ - x~'b| on the fitted rows; ends on a barrier
        for (int it = 0; it < ntiles; ++it) {
            double *xt;
            const double av = open(it, xt);
            if (__double_as_longlong(av) >= 0) {
                double f = 0.0;
                for (int j = 0; j < kt; ++j) f = fma(xt[(size_t)j * ts + tid], bb[j], f);
                put(it, xt, fabs(xt[(size_t)kt * ts + tid] - f));
            }
            if constexpr (!RES) __syncthreads();                   // the next tile overwrites xs
        }
        __syncthreads();
    };
    auto reweigh = [&](const bool ones, const double sc, const bool gram) {   // work <- omega(|r| / sc) (or 1) on the fitted rows [+ the weighted Gram pass]
        for (int it = 0; it < ntiles; ++it) {
            double *xt;
            const double av = open(it, xt);
            if (__double_as_longlong(av) >= 0) put(it, xt, ones ? 1.0 : k11_omega(a.norm, a.c, av / sc));
            else if constexpr (!RES) xt[wc + tid] = av;
            if (gram) {
                __syncthreads();
                accumulate(xt, rows_of(it), true);
            }
            if constexpr (!RES) __syncthreads();
        }
        if (gram) reduce(); else __syncthreads();
    };
    // every work value of the group, in any order, the same trip count in every lane (a key with the sign bit set: no fitted row)
    auto each_key = [&](auto &&f) {
        if constexpr (RES) {
            for (int i = tid; i < ntiles * FIT_TILE; i += 256) f(k11_bits(xs[wc + i]));
        } else {
            for (int64_t r0 = s; r0 < e; r0 += 256 * 8) {          // eight loads in flight per lane
                unsigned long long k[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) { const int64_t r = r0 + j * 256 + tid; k[j] = r < e ? k11_bits(a.rows[r]) : ~0ull; }
#pragma unroll
                for (int j = 0; j < 8; ++j) f(k[j]);
            }
        }
    };
    // one more key in `bin` of the histogram (act: this lane has one).  |r| crowds into a few bins in the exponent passes: the lanes
    // that share the first lane's bin are counted by one ballot and one add, three times over, before the rest add on their own.
    auto count = [&](const int bin, bool act) {
        for (int round = 0; round < 3; ++round) {
            const unsigned long long m = __ballot(act);
            if (!m) break;
            const int leader = __ffsll((long long)m) - 1;
            const int lb = __builtin_amdgcn_readlane(bin, leader);
            const bool same = act && bin == lb;
            const unsigned long long sm = __ballot(same);
            if (lane == leader) atomicAdd(&hist[lb], (int)__popcll(sm));
            act = act && !same;
        }
        if (act) atomicAdd(&hist[bin], 1);
    };
    auto median = [&](const int n) -> double {                     // of the work values with a clear sign bit (n of them); uniform result
        if (tid == 0) { prefix_s = 0; krem_s = (n - 1) / 2; }
        for (int pass = 0; pass < 8; ++pass) {
            const int shift = 56 - 8 * pass;
            hist[tid] = 0;
            __syncthreads();
            const unsigned long long pre = prefix_s;
            each_key([&](const unsigned long long key) {
                count((int)(key >> shift) & 255, !(key >> 63) && (pass == 0 || (key >> (shift + 8)) == pre));
            });
            __syncthreads();
            if (wv == 0) {
                const int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
                const int tot = c0 + c1 + c2 + c3;
                int incl = tot;
                for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
                const int k = krem_s;
                int below = incl - tot;
                if (k >= below && k < incl) {
                    int bin = 0, cnt = c0;
                    if (k >= below + c0) {
                        below += c0; bin = 1; cnt = c1;
                        if (k >= below + c1) {
                            below += c1; bin = 2; cnt = c2;
                            if (k >= below + c2) { below += c2; bin = 3; cnt = c3; }
                        }
                    }
                    prefix_s = (pre << 8) | (unsigned long long)(4 * lane + bin);
                    krem_s = k - below;
                    cnt_s = cnt;
                }
            }
            __syncthreads();
        }
        const unsigned long long vlo = prefix_s;
        if (n & 1) return __longlong_as_double((long long)vlo);
        unsigned long long vhi = vlo;
        if (!(krem_s + 1 < cnt_s)) {                               // (uniform) the upper middle value is the next key up
            if (tid == 0) vmin_s = ~0ull;
            __syncthreads();
            unsigned long long mn = ~0ull;
            each_key([&](const unsigned long long key) {
                if (!(key >> 63) && key > vlo && key < mn) mn = key;
            });
            for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(mn, d); mn = o < mn ? o : mn; }
            if (lane == 0) atomicMin(&vmin_s, mn);
            __syncthreads();
            vhi = vmin_s;
        }
        __syncthreads();                                           // (everyone has read the shared words before the next select resets them)
        return 0.5 * (__longlong_as_double((long long)vlo) + __longlong_as_double((long long)vhi));
    };

    // ---- start: stage, count, the unweighted Gram matrix
    if (tid == 0) { ymax_s = 0; nfit_s = 0; }
    __syncthreads();
    unsigned long long ym = 0;
    for (int it = 0; it < ntiles; ++it) {
        const int64_t t0 = base + (int64_t)it * FIT_TILE;
        double *xt = RES ? xs + (size_t)it * FIT_TILE : xs;
        const bool fit = fit_stage<T, RES>(a, s, e, t0, xt, ts);   // (resident: the one read of the frame, streaming loads)
        put(it, xt, fit ? 1.0 : -1.0);
        const unsigned long long m = __ballot(fit);
        if (lane == 0 && m) atomicAdd(&nfit_s, (int)__popcll(m));
        if (fit) { const unsigned long long yb = k11_bits(fabs(xt[(size_t)kt * ts + tid])); ym = yb > ym ? yb : ym; }
        accumulate(xt, rows_of(it), false);
        if constexpr (!RES) __syncthreads();
    }
    for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(ym, d); ym = o > ym ? o : ym; }
    if (lane == 0) atomicMax(&ymax_s, ym);
    reduce();
    const int n = nfit_s;
    const double ymax = __longlong_as_double((long long)ymax_s);
    int status = POLS_GROUP_OK, iters = 0;
    double sc = fit_nan();
    if (n == 0) status = POLS_GROUP_EMPTY;
    else if (n <= kt) status = POLS_GROUP_FALLBACK;
    else {
        solve();
        if (!ok_s) status = POLS_GROUP_FALLBACK;
        else {
            __syncthreads();
            if (tid < kt) bc[tid] = rhs[tid];
            __syncthreads();
            double sprev = 0.0;
            for (;;) {
                residual(bc);
                sc = median(n) / K11_MAD;
                if (!(sc > 16.0 * FIT_EPS * ymax) || !(sc <= FIT_DBL_MAX)) {   // the scale collapsed: converged where it is
                    if (iters > 0) residual(bp);
                    reweigh(iters == 0, sprev, false);
                    break;
                }
                sprev = sc;
                reweigh(false, sc, true);
                if (tid < kt) bp[tid] = bc[tid];
                solve();
                if (!ok_s) { status = POLS_GROUP_FALLBACK; break; }
                double dmax = 0.0, bmax = 0.0;
                for (int j = 0; j < kt; ++j) { const double bn = rhs[j]; dmax = fmax(dmax, fabs(bn - bc[j])); bmax = fmax(bmax, fabs(bn)); }
                __syncthreads();
                if (tid < kt) bc[tid] = rhs[tid];
                __syncthreads();
                ++iters;
                if (dmax <= a.tol * fmax(bmax, 1e-300)) break;
                if (iters >= a.max_iter) { status = POLS_GROUP_NOT_CONVERGED; break; }
            }
        }
    }
    __syncthreads();
    // ---- outputs
    const bool failed = status == POLS_GROUP_FALLBACK;
    if (tid < kt) {
        const double v = failed ? fit_nan() : (status == POLS_GROUP_EMPTY ? 0.0 : bc[tid]);
        a.coef64[(size_t)g * kt + tid] = v;
        if (a.coef) { if (a.f32) static_cast<float *>(a.coef)[(size_t)g * kt + tid] = (float)v; else static_cast<double *>(a.coef)[(size_t)g * kt + tid] = v; }
    }
    if (tid == 0) {
        if (a.status) a.status[g] = status;
        if (a.scale) a.scale[g] = failed ? fit_nan() : sc;
        if (a.n_iter) a.n_iter[g] = iters;
    }
    if (a.weights && e > s) {                                      // omega of the last update; NaN outside the fit and for a failed group
        T *wo = static_cast<T *>(a.weights);
        const bool al = (reinterpret_cast<uintptr_t>(wo) & 15) == 0;
        const int64_t nch = (e - base + VEC - 1) / VEC;
        for (int64_t c = tid; c < nch; c += 256) {
            const int64_t row0 = base + c * VEC;
            T ov[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const int64_t r = row0 + v;
                double wv_ = -1.0;
                if (r >= s && r < e) wv_ = RES ? xs[wc + (size_t)(r - base)] : a.rows[r];
                ov[v] = (T)((failed || __double_as_longlong(wv_) < 0) ? fit_nan() : wv_);
            }
            if (al && row0 >= s && row0 + VEC <= e) {
                if constexpr (VEC == 4) store_stream(reinterpret_cast<V *>(wo + row0), V{ov[0], ov[1], ov[2], ov[3]});
                else store_stream(reinterpret_cast<V *>(wo + row0), V{ov[0], ov[1]});
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) { const int64_t r = row0 + v; if (r >= s && r < e) wo[r] = ov[v]; }
            }
        }
    }
}

template <typename T, bool RES>
static int k11_launch_t(pols_ctx *ctx, const RlmArgs &a) {
    const size_t lds = k11_lds(a.kt, a.ts);
    if (lds > FIT_LDS_BUDGET) return fail(POLS_ERR_UNSUPPORTED, "rlm: %d columns x %d rows exceed the LDS of a workgroup", a.kt, a.ts);
    static OncePerDevice once;
    return fit_launch(ctx, &k11_rlm_kernel<T, RES>, once, a.n_groups, 256, lds, FIT_LDS_BUDGET, a);
}

int k11_rlm_launch(pols_ctx *ctx, int dtype, const RlmArgs &a, bool resident) {
    if (a.kt < 1 || a.kt > K11_KMAX) return fail(POLS_ERR_UNSUPPORTED, "rlm: %d features (incl. intercept) outside 1..%d", a.kt, K11_KMAX);
    if (a.n_groups == 0) return POLS_OK;
    RlmArgs b = a;
    if (!resident) b.ts = FIT_TS;
    if (dtype == POLS_F32) return resident ? k11_launch_t<float, true>(ctx, b) : k11_launch_t<float, false>(ctx, b);
    return resident ? k11_launch_t<double, true>(ctx, b) : k11_launch_t<double, false>(ctx, b);
}

}  // namespace pols
