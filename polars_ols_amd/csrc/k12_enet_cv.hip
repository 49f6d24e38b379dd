// k12_enet_cv.hip -- K12: elastic-net / lasso regularisation path with K-fold selection of alpha per group (pols_elastic_net_cv).
//
// Per group g, on the rows F_g that pols_least_squares fits (fit_stage: null policy, sqrt(w) scaling, ones column last), n = |F_g|,
// the fitted rows are cut in row order into n_folds contiguous folds (the first n % n_folds hold n / n_folds + 1 rows).  With
// Z = [X~ | y~], fold f has its own Gram matrix Z_f'Z_f = [[G_f, c_f], [c_f', yy_f]]; the training matrix of fold f is the sum of the
// others, the validation error of coefficients b is (yy_f - 2 b'c_f + b'G_f b) / n_f.  So the frame is read once and every one of
// the (n_folds + 1) x n_alphas coordinate-descent fits runs on a kt x kt matrix.  Everything is f64; no floating-point atomics, every
// sum in a fixed order: two runs are bit-identical.
//
// Launches:
//   count      (only when the null policy can remove rows) one workgroup per segment / group: the item's fitted rows, so that
//              every item knows the rank of its first fitted row.  Without it rank = row - group start.
//   fold_gram  one workgroup per segment / group, K10's 256-row tiles (fit_stage, 16-byte column loads).  A wave ballot and a
//              four-entry prefix give every row its rank among the fitted rows, hence its fold; fold ids are monotone down the rows, so a tile
//              is cut into at most n_folds + 1 row ranges [bnd[f], bnd[f + 1]) and the threads -- each owns up to three entries of the packed
//              upper triangle, or one entry of a row partition (tri_spread), as in K10's Gram launch -- sum a range in registers and add it to the
//              thread's own LDS slot of that fold: no branch per row (rows outside the fit are zero in the tile).
//   reduce     (only with segments) per group and entry one wave: lane l sums the segments l, l + 64, ... in order, then a fixed DPP tree.
//   path       one problem = (group, fold) or (group, full data); 16 lanes per problem up to 16 columns, 32 beyond.  Lane l keeps column l
//              of the training matrix (the other folds' matrices summed in fold order) in registers with its own c_l, G_ll and w_l.  The
//              update of coordinate j is one sum over the problem's lanes in which lane j puts -c_j in place of G_jj w_j; only lane j
//              then changes its w.  The candidates are walked in descending order with warm starts; per candidate the fold's own
//              matrix is read once for the validation error and the full problem writes its coef_path row.
//   pick       per group: mean over the folds, the winner (smallest finite score, lowest index on a tie), status, n_iter, the
//              chosen coefficients in f64 for K10's prediction pass.
#include "k12_enet_cv.hpp"
#include "fit_launch.hpp"
#include "fit_tile.inl"

namespace pols {

constexpr size_t K12_LDS_BUDGET = 160 * 1024 - 2048;   // dynamic LDS a launch may ask for (the kernels keep about 1 KB of static LDS beside it)

// first rank of fold f among n fitted rows (f = n_folds: n)
__device__ __forceinline__ int64_t k12_fold_start(int64_t n, int nf, int f) {
    const int64_t q = n / nf, rem = n - q * nf;
    return (int64_t)f * q + min((int64_t)f, rem);
}

// ---------------------------------------------------------------- count
template <typename T>
__global__ void __launch_bounds__(256) k12_count_kernel(const EnetCvArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x;
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    int64_t run = 0;
    for (int64_t it = 0; it < ntiles; ++it) {
        const bool fit = fit_stage<T, false>(a, s, e, base + it * FIT_TILE, dyn, FIT_TS);
        const unsigned long long bal = __ballot(fit);
        if ((tid & 63) == 0) wcnt[tid >> 6] = __popcll(bal);
        __syncthreads();
        run += (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
        __syncthreads();                                           // the next tile overwrites the tile and wcnt
    }
    if (tid == 0) a.item_count[blockIdx.x] = run;
}

// ---------------------------------------------------------------- fold_gram
template <typename T>
__global__ void __launch_bounds__(256) k12_fold_gram_kernel(const EnetCvArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    __shared__ int wcnt[4], bnd[K12_MAX_FOLDS + 1], fold_s[FIT_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, kt = a.kt, nf = a.n_folds;
    constexpr int ts = FIT_TS;
    double *xs = dyn;                                              // (kt + 2) x FIT_TS
    double *facc = xs + (size_t)(kt + 2) * ts;                     // n_folds x sf: a slot per fold and thread entry
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    const TriSpread sp = tri_spread(kt + 1, tid);
    const int ne = sp.ne, parts = sp.parts, sf = parts > 1 ? parts * ne : ne;
    // the group's fitted rows and the rank of this item's first fitted row
    int64_t n, rank0;
    if (a.counted) {
        const int64_t v0 = a.seg_offs ? a.seg_first[g] : g, v1 = a.seg_offs ? a.seg_first[g + 1] : g + 1;
        n = 0; rank0 = 0;
        for (int64_t it = v0; it < v1; ++it) { const int64_t c = a.item_count[it]; if (it < (int64_t)blockIdx.x) rank0 += c; n += c; }
    } else {
        n = a.offs[g + 1] - a.offs[g];
        rank0 = s - a.offs[g];
    }
    const int64_t fq = n / nf, frem = n - fq * nf, fcut = frem * (fq + 1);      // ranks below fcut sit in folds of fq + 1 rows
    for (int q = tid; q < nf * sf; q += 256) facc[q] = 0.0;
    int64_t run = 0;                                               // fitted rows of the tiles behind
    for (int64_t it = 0; it < ntiles; ++it) {
        const int64_t t0 = base + it * FIT_TILE;
        const bool fit = fit_stage<T, false>(a, s, e, t0, xs, ts);
        const int rows_here = (int)min((int64_t)FIT_TILE, e - t0);
        const unsigned long long bal = __ballot(fit);
        if (lane == 0) wcnt[wv] = __popcll(bal);
        if (tid <= nf) bnd[tid] = FIT_TILE;
        __syncthreads();
        int before = __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wv; ++w) before += wcnt[w];
        const int total = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
        int fo = 0;
        if (fq > 0) {                                              // (fewer rows than folds: the group is a fallback, one fold will do)
            const int64_t r = min(rank0 + run + before, n - 1);
            fo = (int)(r < fcut ? r / (fq + 1) : frem + (r - fcut) / fq);
        }
        fold_s[tid] = fo;
        __syncthreads();
        {
            const int prev = tid == 0 ? -1 : fold_s[tid - 1];      // fold ids are monotone down the rows
            for (int f = prev + 1; f <= fo; ++f) bnd[f] = tid;     // first row of the tile whose fold is >= f
        }
        __syncthreads();
        const int flo = fold_s[0], fhi = fold_s[FIT_TILE - 1];
        for (int f = flo; f <= fhi; ++f) {
            double v[3] = {0.0, 0.0, 0.0};
            tri_accumulate(sp, v, xs, ts, bnd[f], min(bnd[f + 1], rows_here));
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (sp.on[q]) facc[f * sf + (parts > 1 ? tid : tid + 256 * q)] += v[q];
        }
        run += total;
        __syncthreads();                                           // the next tile overwrites xs, wcnt, bnd and fold_s
    }
    __syncthreads();
    const size_t gs = k10_gram_stride(kt);
    double *out = a.fold_part + (size_t)blockIdx.x * nf * gs;
    for (int q = tid; q < nf * ne; q += 256) {
        const int f = q / ne, en = q - f * ne;
        double v = 0.0;
        if (parts > 1) { for (int p = 0; p < parts; ++p) v += facc[f * sf + p * ne + en]; }
        else v = facc[f * sf + en];
        out[(size_t)f * gs + en] = v;
    }
    if (tid < nf) {                                                // this item's fitted rows of fold tid
        const int64_t lo = max(rank0, k12_fold_start(n, nf, tid)), hi = min(rank0 + run, k12_fold_start(n, nf, tid + 1));
        out[(size_t)tid * gs + ne] = (double)(hi > lo ? hi - lo : 0);
    }
}

static size_t k12_tile_lds(int kt) { return sizeof(double) * (size_t)(kt + 2) * FIT_TS; }
static size_t k12_fold_lds(int kt, int nf) {
    const int ne = (kt + 1) * (kt + 2) / 2;
    const int sf = ne < 256 ? (256 / ne) * ne : ne;
    return k12_tile_lds(kt) + sizeof(double) * (size_t)nf * sf;
}

template <typename T>
static int k12_count_launch_t(pols_ctx *ctx, const EnetCvArgs &a) {
    static OncePerDevice once;
    return fit_launch(ctx, &k12_count_kernel<T>, once, fit_items(a), 256, k12_tile_lds(a.kt), K12_LDS_BUDGET, a);
}

int k12_count_launch(pols_ctx *ctx, int dtype, const EnetCvArgs &a) {
    if (a.n_groups == 0 || !a.counted) return POLS_OK;
    return dtype == POLS_F32 ? k12_count_launch_t<float>(ctx, a) : k12_count_launch_t<double>(ctx, a);
}

template <typename T>
static int k12_fold_gram_launch_t(pols_ctx *ctx, const EnetCvArgs &a) {
    static OncePerDevice once;
    const int rc = fit_raise_lds(ctx, &k12_fold_gram_kernel<T>, once, K12_LDS_BUDGET);   // (up front: a failure here is reported before the size)
    if (rc) return rc;
    const size_t lds = k12_fold_lds(a.kt, a.n_folds);
    if (lds > K12_LDS_BUDGET) return fail(POLS_ERR_UNSUPPORTED, "elastic_net_cv: %d columns x %d folds exceed the LDS of a workgroup", a.kt, a.n_folds);
    return fit_launch(ctx, &k12_fold_gram_kernel<T>, once, fit_items(a), 256, lds, K12_LDS_BUDGET, a);
}

int k12_fold_gram_launch(pols_ctx *ctx, int dtype, const EnetCvArgs &a) {
    if (a.kt < 1 || a.kt > K12_KMAX) return fail(POLS_ERR_UNSUPPORTED, "elastic_net_cv: %d features (incl. intercept) outside 1..%d", a.kt, K12_KMAX);
    if (a.n_folds < 2 || a.n_folds > K12_MAX_FOLDS) return fail(POLS_ERR_INVALID, "elastic_net_cv: %d folds outside 2..%d", a.n_folds, K12_MAX_FOLDS);
    if (a.n_groups == 0) return POLS_OK;
    return dtype == POLS_F32 ? k12_fold_gram_launch_t<float>(ctx, a) : k12_fold_gram_launch_t<double>(ctx, a);
}

// ---------------------------------------------------------------- reduce
// a workgroup: four entries of one group's fold matrices, one wave each.  Lane l sums the segments l, l + 64, ... in order, then the
// wave's fixed DPP tree: the same order in every run.
__global__ void __launch_bounds__(256) k12_reduce_kernel(const EnetCvArgs a) {
    const size_t per = (size_t)a.n_folds * k10_gram_stride(a.kt), nblk = (per + 3) / 4;
    const int64_t g = blockIdx.x / nblk;
    const int64_t v0 = a.seg_first[g], v1 = a.seg_first[g + 1];
    const size_t q = (size_t)(blockIdx.x - g * nblk) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    double v = 0.0;
    if (q < per)
        for (int64_t it = v0 + lane; it < v1; it += 64) v += a.fold_part[(size_t)it * per + q];
    v = wave_sum_row3(v);
    if (q < per && lane == 63) a.fold_gram[(size_t)g * per + q] = v;
}

int k12_reduce_launch(pols_ctx *ctx, const EnetCvArgs &a) {
    if (a.n_groups == 0 || !a.seg_offs) return POLS_OK;
    const size_t per = (size_t)a.n_folds * k10_gram_stride(a.kt);
    hipLaunchKernelGGL(k12_reduce_kernel, dim3((unsigned)(((per + 3) / 4) * (size_t)a.n_groups)), dim3(256), 0, ctx->stream, a);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

// ---------------------------------------------------------------- path
__device__ __forceinline__ double k12_soft(double x, double thr, bool positive) {   // the reference's soft_threshold
    const double mag = fmax(fabs(x) - thr, 0.0);
    double r = copysign(mag, x);
    if (positive) r = fmax(r, 0.0);
    return r;
}

template <int LPG>
__device__ __forceinline__ double k12_team_sum(double v) {
    v = row_allreduce(v);
    if (LPG == 32) v += __shfl_xor(v, 16);
    return v;
}

template <int LPG>   // lanes per problem = the most columns it handles
__global__ void __launch_bounds__(64) k12_path_kernel(const EnetCvArgs a) {
    const int lane = threadIdx.x, sub = lane & (LPG - 1);
    const int kt = a.kt, nz = kt + 1, ne = nz * (nz + 1) / 2, nf = a.n_folds, na = a.n_alphas;
    const int64_t prob = (int64_t)blockIdx.x * (64 / LPG) + (lane / LPG);
    const bool live = prob < a.n_groups * (nf + 1);
    const int64_t g = live ? prob / (nf + 1) : 0;
    const int p = live ? (int)(prob - g * (nf + 1)) : nf;          // the fold left out; nf: the full-data problem
    const size_t gs = k10_gram_stride(kt);
    const double *FG = a.fold_gram + (size_t)g * nf * gs;
    const bool mine = sub < kt;
    const int su = mine ? sub : 0;

    double n = 0.0;
    for (int f = 0; f < nf; ++f) n += FG[(size_t)f * gs + ne];
    const double n_val = p < nf ? FG[(size_t)p * gs + ne] : 0.0, n_fit = n - n_val;
    double col[LPG];                                               // column `sub` of the training matrix
#pragma unroll
    for (int i = 0; i < LPG; ++i) {
        double v = 0.0;
        if (i < kt && mine) {
            const int at = tri_index(min(i, su), max(i, su), nz);
            for (int f = 0; f < nf; ++f) if (f != p) v += FG[(size_t)f * gs + at];
        }
        col[i] = v;
    }
    double cme = 0.0, dme = 1.0, cfull = 0.0;                      // c_sub and G_sub,sub of the training problem; c_sub of the full data
    if (mine) {
        dme = 0.0;
        const int ac = tri_index(su, kt, nz), ad = tri_index(su, su, nz);
        for (int f = 0; f < nf; ++f) {
            const double c = FG[(size_t)f * gs + ac];
            cfull += c;
            if (f != p) { cme += c; dme += FG[(size_t)f * gs + ad]; }
        }
    }
    double amax = 0.0;
    if (a.automatic) {
        amax = fabs(cfull);
#pragma unroll
        for (int m = 1; m < LPG; m <<= 1) amax = fmax(amax, __shfl_xor(amax, m));
        amax = amax / (n * a.l1_ratio);
    }
    const bool go = live && n > 0.0 && n >= (double)nf && (!a.automatic || (amax > 0.0 && amax < __longlong_as_double(0x7ff0000000000000LL)));
    const double leps = a.automatic ? log(a.eps) : 0.0;
    const bool positive = a.positive != 0;
    const double *VG = FG + (size_t)(p < nf ? p : 0) * gs;         // the validation fold's own matrix
    double wme = 0.0;                                              // w[sub], this lane's own coordinate

    for (int jj = 0; jj < na; ++jj) {
        const int j = a.order[jj];
        const double alpha = a.automatic ? (j == 0 ? amax : amax * exp(leps * ((double)j / (double)(na - 1)))) : a.alphas[j];
        const double an = alpha * n_fit;                           // alpha times the rows of THIS fit
        const double thr = an * a.l1_ratio, l2 = an * (1.0 - a.l1_ratio);
        bool done = !go, stopped = false;
        int sweeps = 0;
        for (int it = 0; it < a.max_iter; ++it) {
            if (__all(done)) break;
            double d2me = 0.0;
#pragma unroll
            for (int c = 0; c < LPG; ++c) {
                if (c < kt) {                                      // (no break: a second exit keeps the loop from unrolling and col[] from registers)
                    // sum_{i != c} G_ci w_i - c_c over the problem's lanes
                    const double sdot = k12_team_sum<LPG>(sub == c ? -cme : col[c] * wme);
                    if (sub == c && !done) {
                        const double wn = k12_soft(-sdot, thr, positive) / (dme + l2);
                        const double dw = wn - wme;
                        d2me = dw * dw;
                        wme = wn;
                    }
                }
            }
            const double d2 = k12_team_sum<LPG>(d2me);
            if (!done) {
                ++sweeps;
                if (sqrt(d2) < a.tol) done = true;
                else if (it + 1 == a.max_iter) stopped = true;
            }
        }
        if (p < nf) {                                              // validation error from the fold's own matrix
            double acc = 0.0;
            for (int i = 0; i < kt; ++i) {
                const double wi = __shfl(wme, i, LPG);
                const double gv = mine ? VG[tri_index(min(i, su), max(i, su), nz)] : 0.0;
                acc = fma(gv, wi, acc);
            }
            const double cv = mine ? VG[tri_index(su, kt, nz)] : 0.0;
            double tot = k12_team_sum<LPG>(mine ? wme * (acc - 2.0 * cv) : 0.0) + VG[ne - 1];
            if (tot < 0.0) tot = 0.0;                              // (a NaN stays a NaN)
            if (live && sub == 0) a.score_part[((size_t)g * nf + p) * na + j] = go ? tot / n_val : fit_nan();
        } else if (live) {
            if (mine) {
                const double v = go ? wme : fit_nan();
                a.path64[((size_t)g * na + j) * kt + sub] = v;
                if (a.coef_path) {
                    if (a.f32) static_cast<float *>(a.coef_path)[((size_t)g * na + j) * kt + sub] = (float)v;
                    else static_cast<double *>(a.coef_path)[((size_t)g * na + j) * kt + sub] = v;
                }
            }
            if (sub == 0) a.grid[(size_t)g * na + j] = (a.automatic && !go) ? fit_nan() : alpha;
        }
        if (live && sub == 0) a.iters[((size_t)g * (nf + 1) + p) * na + j] = sweeps | (stopped ? K12_STOPPED : 0);
    }
}

int k12_path_launch(pols_ctx *ctx, const EnetCvArgs &a) {
    if (a.n_alphas < 1 || a.n_alphas > K12_MAX_ALPHAS) return fail(POLS_ERR_UNSUPPORTED, "elastic_net_cv: %d candidates outside 1..%d", a.n_alphas, K12_MAX_ALPHAS);
    if (a.n_groups == 0) return POLS_OK;
    const int64_t probs = a.n_groups * (a.n_folds + 1);
    if (a.kt <= 16) hipLaunchKernelGGL(k12_path_kernel<16>, dim3((unsigned)((probs + 3) / 4)), dim3(64), 0, ctx->stream, a);
    else hipLaunchKernelGGL(k12_path_kernel<32>, dim3((unsigned)((probs + 1) / 2)), dim3(64), 0, ctx->stream, a);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

// ---------------------------------------------------------------- pick
__global__ void __launch_bounds__(K12_MAX_ALPHAS) k12_pick_kernel(const EnetCvArgs a) {
    __shared__ double sc_s[K12_MAX_ALPHAS];
    __shared__ int best_s;
    const int tid = threadIdx.x, kt = a.kt, nf = a.n_folds, na = a.n_alphas, ne = (kt + 1) * (kt + 2) / 2;
    const int64_t g = blockIdx.x;
    const size_t gs = k10_gram_stride(kt);
    double n = 0.0;
    for (int f = 0; f < nf; ++f) n += a.fold_gram[((size_t)g * nf + f) * gs + ne];
    int sweeps = 0;
    bool stopped = false;
    if (tid < na) {
        double tot = 0.0;
        for (int f = 0; f < nf; ++f) tot += a.score_part[((size_t)g * nf + f) * na + tid];
        const double sc = tot / (double)nf;
        sc_s[tid] = sc;
        if (a.cv_scores) a.cv_scores[(size_t)g * na + tid] = sc;
        for (int p = 0; p <= nf; ++p) {
            const int32_t v = a.iters[((size_t)g * (nf + 1) + p) * na + tid];
            sweeps = max(sweeps, v & (K12_STOPPED - 1));
            stopped = stopped || (v & K12_STOPPED) != 0;
        }
        if (a.n_iter) a.n_iter[(size_t)g * na + tid] = sweeps;
        if (a.alphas_used) a.alphas_used[(size_t)g * na + tid] = a.grid[(size_t)g * na + tid];
    }
    __syncthreads();
    if (tid == 0) {
        int best = -1;
        double bv = 0.0;
        for (int j = 0; j < na; ++j) {
            const double v = sc_s[j];
            if (fabs(v) < __longlong_as_double(0x7ff0000000000000LL) && (best < 0 || v < bv)) { best = j; bv = v; }   // (false for NaN)
        }
        best_s = best;
        if (a.alpha) a.alpha[g] = best >= 0 ? a.grid[(size_t)g * na + best] : fit_nan();
        if (a.alpha_index) a.alpha_index[g] = best;
        if (a.score) a.score[g] = best >= 0 ? bv : fit_nan();
    }
    __syncthreads();
    const int best = best_s;
    if (tid == (best >= 0 ? best : 0) && a.status)
        a.status[g] = best >= 0 ? (stopped ? POLS_GROUP_NOT_CONVERGED : POLS_GROUP_OK) : (n > 0.0 ? POLS_GROUP_FALLBACK : POLS_GROUP_EMPTY);
    if (tid < kt) {
        const double v = best >= 0 ? a.path64[((size_t)g * na + best) * kt + tid] : (n > 0.0 ? fit_nan() : 0.0);
        a.coef64[(size_t)g * kt + tid] = v;
        if (a.coef) {
            if (a.f32) static_cast<float *>(a.coef)[(size_t)g * kt + tid] = (float)v;
            else static_cast<double *>(a.coef)[(size_t)g * kt + tid] = v;
        }
    }
}

int k12_pick_launch(pols_ctx *ctx, const EnetCvArgs &a) {
    if (a.n_groups == 0) return POLS_OK;
    hipLaunchKernelGGL(k12_pick_kernel, dim3((unsigned)a.n_groups), dim3(K12_MAX_ALPHAS), 0, ctx->stream, a);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

}  // namespace pols
