// k16_absorb.hip -- K16: per-group regression that absorbs one categorical effect, the "within" estimator (pols_least_squares_absorb).
//
// Per group g, on the rows F_g that pols_least_squares fits (null policy, a null weight acting as 1e-24), n = |F_g|, the categories
// c = the distinct ids among F_g (C of them), k user columns and never a ones column:
//   W_c = sum_{i in c} w_i,  xbar_c = sum w_i x_i / W_c,  ybar_c likewise (the means FIRST),
//   x~_i = sqrt(w_i) (x_i - xbar_c(i)),  y~_i likewise,  A = X~'X~ (moments of the demeaned rows),  T_jj = sum w_i x_ij^2 (raw),
//   A = L L' where pivot j fails when d_j <= 16 k eps T_jj,  b = A^-1 X~'y~,  e~_i = y~_i - x~_i'b,  RSS = sum e~_i^2 over the rows,
//   a_c = ybar_c - xbar_c'b,  c0 = sum W_c a_c / sum W_c,  df = n - k - C,  sigma2 = RSS / df,
//   V = sigma2 A^-1  |  C / (C - 1) (n - 1) / (n - k - 1) A^-1 (sum_c s_c s_c') A^-1 with s_c = sum_{i in c} e~_i x~_i (only diag V is formed).
// Everything is f64 on the inputs' values, for f32 batches too.  No atomics, every sum in a fixed order: two runs are bit-identical.
//
// Launches:
//   order    K7c's builder (k7c_order_launch): the probe, and K9's radix passes when an id decreases inside a group.  In the order it
//            gives, a category is a run of equal ids and a group's categories come in ascending id.
//   count    one workgroup per segment of a long group (ensure_segments) or per group: the run starts inside the item; then one
//            workgroup takes the exclusive prefix over the items.  The total goes back to the host (one synchronise) and sizes the table.
//   index    per item: the category of every position = the prefix of its item + the run starts up to it (ballot / popcount per
//            256-position tile), stored per ROW in frame order (int32); the thread of a run start stores the category's first position.
//   means    one wave per category: lane l takes positions l, l + 64, ..; per 64 positions the k + 3 terms (1, w, w y, w x_j) are summed
//            over the wave by DPP and added to the accumulator of the lane that owns the term: batches in position order.
//   gram     per item, frame order: 256-row tiles staged by fit_stage (16-byte streaming loads, null policy, sqrt(w)); the raw T_jj
//            are accumulated from the staged tile, then the thread of a row subtracts sqrt(w) times its category's means (a gather
//            from the table) and the (k + 1)(k + 2) / 2 entries of [X~ | y~]'[X~ | y~] are accumulated with the family's TriSpread.
//   solve    one wave per group: partials in segment order (a non-finite moment fails the group), C and the between sum of squares from
//            the table, fit_chol_factor against T, the two substitutions, A^-1 through the inverse of the factor, then a_c into the
//            table (lane l takes categories l, l + 64, ..) and c0.  coef, status, n_obs, n_categories are final here.
//   resid    one wave per category, positions as in `means`: e~_i from the row's own values, sum e~_i^2; cluster: s_c by the same DPP
//            sums, z = A^-1 s_c, the k squares z_j^2.  Not launched when no wanted output needs a residual.
//   finish   one wave per group: RSS (and sum_c z_cj^2) over the group's categories in ascending order, sigma2, se / t / p, r2_within, r2.
//   predict  per item, fit_predict_rows: pred = x_i'b + a_c, resid = y - pred, fe = a_c - c0 for every row of the frame.
#include "k16_absorb.hpp"
#include "fit_launch.hpp"
#include "k16_absorb.inl"

#include <algorithm>

namespace pols {

__device__ __forceinline__ int64_t k16_row(const AbsorbArgs &a, int64_t i) { return a.order ? (int64_t)a.order[i] : i; }
// a category starts at position i: a group start, or another id than position i - 1
__device__ __forceinline__ bool k16_starts(const AbsorbArgs &a, int64_t gs, int64_t i) {
    if (i == gs) return true;
    return a.ids[k16_row(a, i)] != a.ids[k16_row(a, i - 1)];
}
// the item of a workgroup of the count / index launches (no tile grid)
__device__ __forceinline__ void k16_item(const AbsorbArgs &a, int64_t &g, int64_t &gs, int64_t &s, int64_t &e) {
    const int64_t sgi = blockIdx.x;
    g = a.seg_offs ? (int64_t)a.seg_map[sgi] : sgi;
    gs = a.offs[g];
    s = a.seg_offs ? a.seg_offs[sgi] : gs;
    e = a.seg_offs ? a.seg_offs[sgi + 1] : a.offs[g + 1];
}
// ---------------------------------------------------------------- count, scan, index
__global__ void __launch_bounds__(256) k16_count_kernel(const AbsorbArgs a) {
    __shared__ int red[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t g, gs, s, e;
    k16_item(a, g, gs, s, e);
    int cnt = 0;
    for (int64_t i = s + tid; i < e; i += 256) cnt += k16_starts(a, gs, i) ? 1 : 0;
    for (int off = 32; off; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) red[wv] = cnt;
    __syncthreads();
    if (tid == 0) a.item_cnt[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(256) k16_scan_kernel(const int32_t *cnt, const int64_t n, int64_t *first) {
    __shared__ int64_t sh[256];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += 256) {
        const int64_t i = base + tid;
        const int64_t v = i < n ? (int64_t)cnt[i] : 0;
        sh[tid] = v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int64_t t = tid >= off ? sh[tid - off] : 0;
            __syncthreads();
            sh[tid] += t;
            __syncthreads();
        }
        if (i < n) first[i] = carry + sh[tid] - v;
        carry += sh[255];
        __syncthreads();
    }
    if (tid == 0) first[n] = carry;
}

__global__ void __launch_bounds__(256) k16_index_kernel(const AbsorbArgs a) {
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t g, gs, s, e;
    k16_item(a, g, gs, s, e);
    if (blockIdx.x == 0 && tid == 0) a.cat_start[a.n_cats] = a.offs[a.n_groups];
    const int64_t first = a.item_first[blockIdx.x];
    int64_t running = 0;                                           // run starts of the tiles before
    for (int64_t tb = s; tb < e; tb += 256) {
        const int64_t i = tb + tid;
        const bool st = i < e && k16_starts(a, gs, i);
        const unsigned long long m = __ballot(st);
        if (lane == 0) wcnt[wv] = __popcll(m);
        __syncthreads();
        int before = 0, nst = 0;
        for (int q = 0; q < 4; ++q) { before += q < wv ? wcnt[q] : 0; nst += wcnt[q]; }
        if (i < e) {
            // (a segment that begins inside a run: first - 1, the last category that started before it)
            const int64_t c = first + running + before + __popcll(m & ((1ull << lane) - 1ull)) + (st ? 1 : 0) - 1;
            a.catidx[k16_row(a, i)] = (int32_t)c;
            if (st) a.cat_start[c] = i;
        }
        running += nst;
        __syncthreads();
    }
}

int k16_count_launch(pols_ctx *ctx, const AbsorbArgs &a) {
    const int64_t items = fit_items(a);
    if (items == 0) return POLS_OK;
    hipLaunchKernelGGL(k16_count_kernel, dim3((unsigned)items), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k16_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, (const int32_t *)a.item_cnt, items, a.item_first);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

int k16_index_launch(pols_ctx *ctx, const AbsorbArgs &a) { return fit_launch_plain(ctx, k16_index_kernel, fit_items(a), 256, 0, a); }

// ---------------------------------------------------------------- means
template <typename T>
__global__ void __launch_bounds__(64) k16_means_kernel(const AbsorbArgs a) {
    __shared__ const void *xp[POLS_MAX_FEATURES];
    const int lane = threadIdx.x, k = a.k_user, pol = a.null_policy;
    const int64_t c = blockIdx.x, p0 = a.cat_start[c], p1 = a.cat_start[c + 1];
    k16_columns(a, xp, lane);
    __syncthreads();
    const T *yp = static_cast<const T *>(a.y), *wp = static_cast<const T *>(a.w);
    double acc = 0.0;                                              // lane 0: n_c, 1: W_c, 2: sum w y, 3 + j: sum w x_j
    for (int64_t pb = p0; pb < p1; pb += 64) {
        const int64_t p = pb + lane;
        const bool live = p < p1;
        const int64_t r = live ? k16_row(a, p) : 0;
        const bool fit = live && null_row_in_fit<T>(pol, a.valid, a.y, xp, k, r);
        const double wv = !fit ? 0.0 : (wp ? (double)wp[r] : 1.0);
        double t = k16_wave_sum(fit ? 1.0 : 0.0);
        if (lane == 0) acc += t;
        t = k16_wave_sum(wv);
        if (lane == 1) acc += t;
        t = k16_wave_sum(fit ? wv * (double)null_fill<T>(pol, yp[r]) : 0.0);
        if (lane == 2) acc += t;
        for (int j = 0; j < k; ++j) {
            t = k16_wave_sum(fit ? wv * (double)null_fill<T>(pol, static_cast<const T *>(xp[j])[r]) : 0.0);
            if (lane == 3 + j) acc += t;
        }
    }
    const double nc = __shfl(acc, 0), W = __shfl(acc, 1);
    double *m = a.cat + (size_t)c * k16_cat_stride(k);
    if (lane < 2) m[lane] = acc;
    else if (lane < 3 + k) m[lane] = nc > 0.0 ? acc / W : fit_nan();
}

int k16_means_launch(pols_ctx *ctx, int dtype, const AbsorbArgs &a) {
    return dtype == POLS_F32 ? fit_launch_plain(ctx, k16_means_kernel<float>, a.n_cats, 64, 0, a)
                             : fit_launch_plain(ctx, k16_means_kernel<double>, a.n_cats, 64, 0, a);
}

// ---------------------------------------------------------------- gram
template <typename T>
__global__ void __launch_bounds__(256) k16_gram_kernel(const AbsorbArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = a.k_user, nz = k + 1, ne = nz * (nz + 1) / 2;
    constexpr int ts = FIT_TS;
    double *xs = dyn;                                              // (k + 3) x ts: x (-> x~), sqrt(w) (-> y~), y~, the raw weights
    double *gp = xs + (size_t)(k + 3) * ts;                        // 256
    double *red = gp + 256;                                        // 4
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    const TriSpread sp = tri_spread(nz, tid);
    double acc[3] = {0.0, 0.0, 0.0};
    const int P = 256 / k, tp = tid / k, tj = tid - tp * k;        // thread (row partition tp, column tj) of the raw second moments
    const bool ton = tp < P;
    double tacc = 0.0, cnt = 0.0;
    const size_t cs = k16_cat_stride(k);
    for (int64_t it = 0; it < ntiles; ++it) {
        const int64_t t0 = base + it * FIT_TILE;
        const bool fit = fit_stage<T, true>(a, s, e, t0, xs, ts);
        const int nr = (int)min((int64_t)FIT_TILE, e - t0);
        if (ton) {
            const double *cj = xs + (size_t)tj * ts;
            for (int r = tp; r < nr; r += P) tacc = fma(cj[r], cj[r], tacc);
        }
        __syncthreads();
        double yt = 0.0;
        if (fit) {
            const double *m = a.cat + (size_t)a.catidx[t0 + tid] * cs;
            const double sw = xs[(size_t)k * ts + tid];
            for (int c = 0; c < k; ++c) xs[(size_t)c * ts + tid] = fma(-sw, m[3 + c], xs[(size_t)c * ts + tid]);
            yt = fma(-sw, m[2], xs[(size_t)(k + 1) * ts + tid]);
            cnt += 1.0;
        }
        xs[(size_t)k * ts + tid] = yt;                             // y~ beside x~: the nz columns of the cross-product
        __syncthreads();
        tri_accumulate(sp, acc, xs, ts, 0, nr);
        __syncthreads();                                           // the next tile overwrites xs
    }
    double *out = a.gram_part + (size_t)blockIdx.x * k16_gram_stride(k);
    tri_reduce(sp, acc, gp, out);
    if (ton) gp[tid] = tacc;                                       // (tid = tp k + tj)
    __syncthreads();
    if (tid < k) {
        double v = 0.0;
        for (int p = 0; p < P; ++p) v += gp[p * k + tid];
        out[ne + tid] = v;
    }
    const double tot = fit_block_sum(cnt, red, lane, wv);
    if (tid == 0) out[ne + k] = tot;
}

static size_t k16_gram_lds(int k) { return sizeof(double) * ((size_t)(k + 3) * FIT_TS + 256 + 4); }

template <typename T>
static int k16_gram_launch_t(pols_ctx *ctx, const AbsorbArgs &a) {
    const size_t lds = k16_gram_lds(a.k_user);
    if (lds > FIT_LDS_BUDGET) return fail(POLS_ERR_UNSUPPORTED, "absorb: %d columns exceed the LDS of a workgroup", a.k_user);
    static OncePerDevice once;
    return fit_launch(ctx, &k16_gram_kernel<T>, once, fit_items(a), 256, lds, FIT_LDS_BUDGET, a);
}

int k16_gram_launch(pols_ctx *ctx, int dtype, const AbsorbArgs &a) {
    if (fit_items(a) == 0) return POLS_OK;
    return dtype == POLS_F32 ? k16_gram_launch_t<float>(ctx, a) : k16_gram_launch_t<double>(ctx, a);
}

// ---------------------------------------------------------------- solve
__global__ void __launch_bounds__(64) k16_solve_kernel(const AbsorbArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int lane = threadIdx.x, k = a.k_user, nz = k + 1, ne = nz * (nz + 1) / 2, kc = k + a.icpt;
    const AbsorbLds o = k16_lds(k);
    double *Gs = dyn + o.Gs, *rhs = dyn + o.rhs;
    const int64_t g = blockIdx.x;
    int64_t v0, v1;
    fit_group_items(a, g, v0, v1);
    const size_t cs = k16_cat_stride(k);
    const bool finite = fit_sum_parts(a.gram_part, k16_gram_stride(k), v0, v1, ne + k + 1, Gs, lane);   // the triangle, T_jj, n
    fit_wave_sync();
    const double n = Gs[ne + k];
    // the group's categories: those with a fitted row count; the weighted mean of y and the between sum of squares from the table
    const int64_t c0i = a.item_first[v0], c1i = a.item_first[v1];
    double lC = 0.0, lW = 0.0, lWy = 0.0;
    for (int64_t c = c0i + lane; c < c1i; c += 64) {
        const double *m = a.cat + (size_t)c * cs;
        if (m[0] > 0.0) { lC += 1.0; lW += m[1]; lWy = fma(m[1], m[2], lWy); }
    }
    const double C = k16_wave_sum(lC), W = k16_wave_sum(lW), ybar = k16_wave_sum(lWy) / W;
    double lB = 0.0;
    for (int64_t c = c0i + lane; c < c1i; c += 64) {
        const double *m = a.cat + (size_t)c * cs;
        if (m[0] > 0.0) { const double d = m[2] - ybar; lB = fma(m[1] * d, d, lB); }
    }
    const double yy = Gs[tri_index(k, k, nz)], tss = yy + k16_wave_sum(lB);
    const double df = n - (double)k - C;
    bool ok = finite && n > 0.0 && df > 0.0;
    double *st = a.state + (size_t)g * k16_state_stride(k);
    ok = k16_solve_core(ok, dyn, o, st + 8 + k, k, lane);
    // the effects a_c = ybar_c - xbar_c'b into the table (NaN for a category without a fitted row, and for a group without a fit)
    double lA = 0.0;
    for (int64_t c = c0i + lane; c < c1i; c += 64) {
        double *m = a.cat + (size_t)c * cs;
        const bool has = m[0] > 0.0;
        double ac = fit_nan();
        if (ok && has) {
            ac = m[2];
            for (int j = 0; j < k; ++j) ac = fma(-m[3 + j], rhs[j], ac);
            lA = fma(m[1], ac, lA);
        }
        m[0] = ac;
    }
    const double c0 = a.icpt ? k16_wave_sum(lA) / W : 0.0;
    if (lane == 0) {
        st[0] = n; st[1] = ok ? 1.0 : 0.0; st[2] = C; st[3] = df; st[4] = ok ? c0 : fit_nan(); st[5] = yy; st[6] = tss; st[7] = W;
        if (a.status) a.status[g] = !(n > 0.0) ? POLS_GROUP_EMPTY : (!(df > 0.0) ? POLS_GROUP_BAD_DOF : (ok ? POLS_GROUP_OK : POLS_GROUP_FALLBACK));
        if (a.n_obs) a.n_obs[g] = (int64_t)n;
        if (a.n_categories) a.n_categories[g] = (int64_t)C;
    }
    const double fillv = n > 0.0 ? fit_nan() : 0.0;                // no rows: zeros, as the existing entries
    if (lane < k) st[8 + lane] = ok ? rhs[lane] : fit_nan();
    if (lane < kc) fit_store_coef(a, g, kc, lane, ok ? (lane < k ? rhs[lane] : c0) : fillv);
}

int k16_solve_launch(pols_ctx *ctx, const AbsorbArgs &a) {
    return fit_launch_plain(ctx, k16_solve_kernel, a.n_groups, 64, sizeof(double) * (size_t)k16_lds(a.k_user).total, a);
}

// ---------------------------------------------------------------- resid
template <typename T>
__global__ void __launch_bounds__(64) k16_resid_kernel(const AbsorbArgs a) {
    __shared__ const void *xp[POLS_MAX_FEATURES];
    __shared__ double bs[K16_KMAX], ms[K16_KMAX], ss[K16_KMAX], Ai[K16_KMAX * K16_KMAX];
    const int lane = threadIdx.x, k = a.k_user, pol = a.null_policy;
    const bool cluster = a.cluster != 0;
    const int64_t c = blockIdx.x, p0 = a.cat_start[c], p1 = a.cat_start[c + 1];
    const int64_t g = k16_group_of(a.offs, a.n_groups, p0);
    const double *st = a.state + (size_t)g * k16_state_stride(k);
    const double *m = a.cat + (size_t)c * k16_cat_stride(k);
    double *out = a.resid_part + (size_t)c * k16_resid_stride(k, cluster);
    if (!absorb_resid_head(st, 8, 8 + k, out, cluster, k, lane, bs, Ai)) return;
    k16_columns(a, xp, lane);
    if (lane < k) ms[lane] = m[3 + lane];
    __syncthreads();
    const T *yp = static_cast<const T *>(a.y), *wp = static_cast<const T *>(a.w);
    const double ybar = m[2];
    double rss = 0.0, sacc = 0.0;                                  // sacc, lane j < k: s_cj
    for (int64_t pb = p0; pb < p1; pb += 64) {
        const int64_t p = pb + lane;
        const bool live = p < p1;
        const int64_t r = live ? k16_row(a, p) : 0;
        const bool fit = live && null_row_in_fit<T>(pol, a.valid, a.y, xp, k, r);
        double ev = 0.0, sw = 0.0;
        if (fit) {
            sw = wp ? sqrt((double)wp[r]) : 1.0;
            double f = (double)null_fill<T>(pol, yp[r]) - ybar;
            for (int j = 0; j < k; ++j) f = fma(-((double)null_fill<T>(pol, static_cast<const T *>(xp[j])[r]) - ms[j]), bs[j], f);
            ev = sw * f;
        }
        rss = fma(ev, ev, rss);
        if (cluster) {
            for (int j = 0; j < k; ++j) {
                const double u = fit ? ev * (sw * ((double)null_fill<T>(pol, static_cast<const T *>(xp[j])[r]) - ms[j])) : 0.0;
                const double t = k16_wave_sum(u);
                if (lane == j) sacc += t;
            }
        }
    }
    absorb_resid_tail(rss, sacc, ss, Ai, out, cluster, k, lane);
}

int k16_resid_launch(pols_ctx *ctx, int dtype, const AbsorbArgs &a) {
    return dtype == POLS_F32 ? fit_launch_plain(ctx, k16_resid_kernel<float>, a.n_cats, 64, 0, a)
                             : fit_launch_plain(ctx, k16_resid_kernel<double>, a.n_cats, 64, 0, a);
}

// ---------------------------------------------------------------- finish
__global__ void __launch_bounds__(64) k16_finish_kernel(const AbsorbArgs a) {
    const int k = a.k_user;
    const int64_t g = blockIdx.x;
    int64_t v0, v1;
    fit_group_items(a, g, v0, v1);
    const double *st = a.state + (size_t)g * k16_state_stride(k);
    const double n = st[0], C = st[2];
    absorb_finish(a, g, st, a.item_first[v0], a.item_first[v1], k16_resid_stride(k, a.cluster != 0), C, n - (double)k - 1.0, 8, 8 + k);
}

int k16_finish_launch(pols_ctx *ctx, const AbsorbArgs &a) { return fit_launch_plain(ctx, k16_finish_kernel, a.n_groups, 64, 0, a); }

// ---------------------------------------------------------------- predict
template <typename T>
__global__ void __launch_bounds__(256) k16_predict_kernel(const AbsorbArgs a) {
    const int k = a.k_user;
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    if (e <= s) return;
    const double *st = a.state + (size_t)g * k16_state_stride(k);
    const double c0 = st[4];
    const size_t cs = k16_cat_stride(k);
    T *const out[3] = {static_cast<T *>(a.pred), static_cast<T *>(a.resid), static_cast<T *>(a.fe)};
    fit_predict_rows<T>(a, s, e, base, st + 8, 0.0, (const T *)nullptr, out,
                        [&](const double lin, const double yv, const int64_t r, const bool in, const bool fit, double (&o)[3]) {
                            const double ac = (in && fit) ? a.cat[(size_t)a.catidx[r] * cs] : fit_nan();
                            const double pr = lin + ac;
                            o[0] = pr;
                            o[1] = yv - pr;
                            o[2] = ac - c0;
                        });
}

int k16_predict_launch(pols_ctx *ctx, int dtype, const AbsorbArgs &a) {
    if (a.n_groups == 0 || a.n_rows == 0 || (!a.pred && !a.resid && !a.fe)) return POLS_OK;
    return dtype == POLS_F32 ? fit_launch_plain(ctx, k16_predict_kernel<float>, fit_items(a), 256, 0, a)
                             : fit_launch_plain(ctx, k16_predict_kernel<double>, fit_items(a), 256, 0, a);
}

}  // namespace pols
