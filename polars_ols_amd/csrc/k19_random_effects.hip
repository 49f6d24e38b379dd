// k19_random_effects.hip -- K19: per-group random-effects panel regression with the Hausman test (pols_random_effects).
//
// Per group g, on the rows K16 fits (no weights), the categories c with T_c fitted rows (C of them), k user columns, kc = k + intercept,
// zbar_c = (xbar_c, 1) or xbar_c:
//   within    K16 unchanged: b_w, A_w = X~'X~, X~'y~, RSS_w from the rows, df_w = n - k - C, sigma2_e = RSS_w / df_w.
//   between   B = sum_c zbar_c zbar_c', b_b = B^-1 sum_c zbar_c ybar_c (pivot j fails when d_j <= 16 kc eps B_jj),
//             RSS_b = sum_c (ybar_c - zbar_c'b_b)^2 from the table, df_b = C - kc.
//   variance  Tbar = C / sum_c (1 / T_c), sigma2_u = max(0, RSS_b / df_b - sigma2_e / Tbar), theta_c = 1 - sqrt(sigma2_e / (sigma2_e + T_c sigma2_u)).
//   GLS       q_c = T_c (1 - theta_c)^2, M = embed(A_w) + sum_c q_c zbar_c zbar_c', v = embed(X~'y~) + sum_c q_c zbar_c ybar_c, b = M^-1 v
//             (pivot j fails when d_j <= 16 kc eps T_jj, the raw second moment, n for the intercept).
//   RSS       sum_i (y~_i - x~_i'b)^2 from the rows + sum_c q_c (ybar_c - zbar_c'b)^2 from the table, df = n - kc, V = RSS / df M^-1.
//   Hausman   d = b_w - b_1..k, D = sigma2_e (A_w^-1 - (M^-1)_1..k,1..k), H = d'D^-1 d, p = Q(k / 2, H / 2); NaN when a pivot of D is not positive.
//   effects   u_c = T_c sigma2_u / (T_c sigma2_u + sigma2_e) (ybar_c - zbar_c'b).
// Everything is f64.  No atomics, every sum in a fixed order: two runs, and the two routes of the table kernel, are bit-identical.
//
// Launches (behind K16's index, means, gram, solve, resid and finish, which give the table, the within moments, b_w, A_w^-1, sigma2_e):
//   rows     one thread per group: the rows of K16's table the group spans (the host splits the frame into the two routes by them).
//   table    one 256-thread workgroup per group, the whole chain above.  A sum over the table's rows has two shapes.  An entry of a packed
//            triangle ((kc + 1)(kc + 2) / 2 entries, ybar as the last column): P = 256 / entries partitions (1 beyond 256 entries), partition
//            p sums rows p, p + P, .. in row order, the partitions meet in partition order, the within moment is added last.  A scalar
//            (RSS_b, sum 1 / T_c, the table's part of RSS): thread t sums rows t, t + 256, .., then fit_block_sum.  The one-wave pieces
//            (fit_chol_solve, k16_solve_core, fit_chol_factor) run in wave 0 between barriers.  RESIDENT: the group's rows of the table and
//            the q_c are in LDS (sized by the frame's largest resident group); GLOBAL: both are read where they lie in global memory.  The
//            code, the partitions and the order of every sum are the same, so the routes agree bit for bit.
//   resid    K16's resid launch on a state row that holds b: the row term of RSS per category.  Only when se / t / p are wanted.
//   finish   one wave per group: the row terms in K16's finish order (lane l takes categories l, l + 64, ..) + the table's part, sigma2, se / t / p.
//   predict  per item, fit_predict_rows: pred = z_i'b, resid = y - pred, the row's u_c and theta_c.
#include "k19_random_effects.hpp"
#include "fit_launch.hpp"
#include "k16_absorb.hpp"
#include "k16_absorb.inl"

namespace pols {

// entry i of (zbar_c, ybar_c) from row m of K16's table: the k means, the one of the intercept, ybar at column kc
__device__ __forceinline__ double k19_z(const double *m, const int i, const int k, const int kc) { return i < k ? m[3 + i] : (i < kc ? 1.0 : m[2]); }

// whether v[0 .. n) are all finite, the same in every lane; all 64 lanes of one wave call it
__device__ __forceinline__ bool k19_finite(const double *v, const int n, const int lane) {
    bool f = true;
    for (int i = lane; i < n; i += 64) f = f && fabs(v[i]) <= FIT_DBL_MAX;
    return __ballot(!f) == 0;
}

// Gs[en], en an entry (i, j) of the packed upper triangle over (zbar, ybar): the sum over the table's rows with T_c > 0 of w_c z_ci z_cj,
// w_c = 1 (qv == nullptr) or qv[c]; with qv the within moments Gw are embedded.  256 threads; part: max(256, entries) doubles.  Ends on
// a barrier.
__device__ __forceinline__ void k19_table_sum(const double *tab, const int64_t rows, const double *qv, const double *Gw, double *part, double *Gs,
                                              const int k, const int kc) {
    const int tid = threadIdx.x, nz = kc + 1, ne = nz * (nz + 1) / 2, P = ne < 256 ? 256 / ne : 1;
    const size_t cs = k16_cat_stride(k);
    for (int idx = tid; idx < P * ne; idx += 256) {
        const int p = idx / ne, en = idx - p * ne;
        int i, j;
        tri_unpack(en, nz, i, j);
        double v = 0.0;
        for (int64_t c = p; c < rows; c += P) {
            const double *m = tab + (size_t)c * cs;
            if (!(m[1] > 0.0)) continue;
            const double zi = k19_z(m, i, k, kc), zj = k19_z(m, j, k, kc);
            v = qv ? fma(qv[c] * zi, zj, v) : fma(zi, zj, v);
        }
        part[idx] = v;
    }
    __syncthreads();
    for (int en = tid; en < ne; en += 256) {
        double v = 0.0;
        for (int p = 0; p < P; ++p) v += part[p * ne + en];
        if (qv) {
            int i, j;
            tri_unpack(en, nz, i, j);
            if (j < k) v += Gw[tri_index(i, j, k + 1)];                      // embed(A_w)
            else if (i < k && j == kc) v += Gw[tri_index(i, k, k + 1)];      // embed(X~'y~)
        }
        Gs[en] = v;
    }
    __syncthreads();
}

// ybar_c - zbar_c'b of row m
__device__ __forceinline__ double k19_table_resid(const double *m, const double *b, const int k, const int kc) {
    double r = m[2];
    for (int j = 0; j < kc; ++j) r = fma(-k19_z(m, j, k, kc), b[j], r);
    return r;
}

__global__ void __launch_bounds__(256) k19_rows_kernel(const RandomEffectsArgs a) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.n_groups) return;
    int64_t v0, v1;
    fit_group_items(a, g, v0, v1);
    a.table_rows[g] = a.item_first[v1] - a.item_first[v0];
}

int k19_rows_launch(pols_ctx *ctx, const RandomEffectsArgs &a) { return fit_launch_plain(ctx, k19_rows_kernel, (a.n_groups + 255) / 256, 256, 0, a); }

// ---------------------------------------------------------------- table
template <bool RES>
__global__ void __launch_bounds__(256) k19_table_kernel(const RandomEffectsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = a.k_user, kc = a.kt, nz = kc + 1, ne = nz * (nz + 1) / 2, nw = (k + 1) * (k + 2) / 2;
    const K19Lds o = k19_lds(k, kc, RES ? a.res_rows : 0);
    const int64_t g = a.list ? (int64_t)a.list[blockIdx.x] : (int64_t)blockIdx.x;
    int64_t v0, v1;
    fit_group_items(a, g, v0, v1);
    const int64_t c0i = a.item_first[v0], rows = a.item_first[v1] - c0i;
    const size_t cs = k16_cat_stride(k);
    const double *tab = a.cat + (size_t)c0i * cs;
    double *qv = a.q_c + c0i;
    if (RES) {                                                     // (the host's split: rows <= a.res_rows)
        for (int64_t i = tid; i < rows * (int64_t)cs; i += 256) dyn[o.tab + i] = tab[i];
        tab = dyn + o.tab;
        qv = dyn + o.q;
    }
    double *Gw = dyn + o.Gw, *Gs = dyn + o.Gs, *rhs = dyn + o.rhs, *Minv = dyn + o.Minv, *bb = dyn + o.bb, *sc = dyn + o.sc, *red = dyn + o.red;
    double *part = dyn + o.part;
    const double *ws = a.wstate + (size_t)g * k16_state_stride(k);
    const double n = ws[0], C = ws[2], dfw = ws[3], dfb = C - (double)kc, s2e = a.sigma2_e[g], q = fit_nan();
    if (wv == 0) {
        const bool fin = fit_sum_parts(a.gram_part, k16_gram_stride(k), v0, v1, nw + k + 1, Gw, lane);   // the triangle, T_jj, n
        if (lane == 0) sc[0] = fin ? 1.0 : 0.0;
    }
    __syncthreads();
    bool ok = sc[0] != 0.0 && ws[1] != 0.0 && n > 0.0 && dfw > 0.0 && dfb > 0.0;   // (workgroup-uniform, as every `ok` below)
    // between
    if (ok) {
        k19_table_sum(tab, rows, nullptr, Gw, part, Gs, k, kc);
        if (wv == 0) {
            const bool s = k19_finite(Gs, ne, lane) && fit_chol_solve(Gs, dyn + o.A, rhs, dyn + o.d0, kc, lane);
            if (lane < kc) bb[lane] = rhs[lane];
            if (lane == 0) sc[1] = s ? 1.0 : 0.0;
        }
        __syncthreads();
        ok = sc[1] != 0.0;
    }
    // variance components, theta_c, q_c
    double s2u = q;
    if (ok) {
        double l = 0.0, li = 0.0;
        for (int64_t c = tid; c < rows; c += 256) {
            const double *m = tab + (size_t)c * cs;
            if (!(m[1] > 0.0)) continue;
            const double r = k19_table_resid(m, bb, k, kc);
            l = fma(r, r, l);
            li += 1.0 / m[1];
        }
        const double rssb = fit_block_sum(l, red, lane, wv), sinv = fit_block_sum(li, red, lane, wv);
        const double raw = rssb / dfb - s2e / (C / sinv);
        ok = fabs(raw) <= FIT_DBL_MAX;
        s2u = raw > 0.0 ? raw : 0.0;
    }
    if (ok) {
        for (int64_t c = tid; c < rows; c += 256) {
            const double Tc = tab[(size_t)c * cs + 1];
            double th = q, qc = 0.0;
            if (Tc > 0.0) {
                th = 1.0 - sqrt(s2e / fma(Tc, s2u, s2e));
                qc = Tc * ((1.0 - th) * (1.0 - th));
            }
            qv[c] = qc;
            a.theta_c[c0i + c] = th;
        }
        __syncthreads();
        // GLS
        k19_table_sum(tab, rows, qv, Gw, part, Gs, k, kc);
        if (wv == 0) {
            if (lane < kc) dyn[o.T + lane] = lane < k ? Gw[nw + lane] : n;   // the pivots are held against the RAW second moments
            fit_wave_sync();
            const AbsorbLds so = {o.Gs, o.T, o.A, o.d0, o.rhs, o.Ri, 0};
            const bool s = k16_solve_core(k19_finite(Gs, ne, lane), dyn, so, Minv, kc, lane);
            if (lane == 0) sc[2] = s ? 1.0 : 0.0;
        }
        __syncthreads();
        ok = sc[2] != 0.0;
    }
    // the table's part of RSS, the effects
    double rsst = q;
    if (ok) {
        double l = 0.0;
        for (int64_t c = tid; c < rows; c += 256) {
            const double *m = tab + (size_t)c * cs;
            double u = q;
            if (m[1] > 0.0) {
                const double r = k19_table_resid(m, rhs, k, kc), tu = m[1] * s2u;
                l = fma(qv[c] * r, r, l);
                u = tu / (tu + s2e) * r;
            }
            a.u_c[c0i + c] = u;
        }
        rsst = fit_block_sum(l, red, lane, wv);
        ok = fabs(rsst) <= FIT_DBL_MAX;
    }
    if (!ok)
        for (int64_t c = tid; c < rows; c += 256) { a.theta_c[c0i + c] = q; a.u_c[c0i + c] = q; }
    if (wv != 0) return;
    // Hausman: D = sigma2_e (A_w^-1 - (M^-1)_1..k,1..k) = L L', H = |L^-1 (b_w - b)|^2
    double H = q, Hp = q;
    if (ok) {
        double *D = dyn + o.D, *dz = dyn + o.dz, *dv = dyn + o.dv;
        const int LD = k + 1;
        for (int p = lane; p < k * k; p += 64) {
            const int i = p / k, j = p - i * k;
            D[i * LD + j] = s2e * (ws[8 + k + p] - Minv[i * kc + j]);
        }
        if (lane < k) { dz[lane] = 0.0; dv[lane] = ws[8 + lane] - rhs[lane]; }
        fit_wave_sync();
        if (fit_chol_factor(D, dz, k, lane)) {
            for (int j = 0; j < k; ++j) {                          // L z = d
                const double z = dv[j] / D[j * LD + j];
                fit_wave_sync();
                if (lane == j) dv[j] = z;
                else if (lane > j && lane < k) dv[lane] -= D[lane * LD + j] * z;
                fit_wave_sync();
            }
            H = 0.0;
            for (int j = 0; j < k; ++j) H = fma(dv[j], dv[j], H);
            Hp = k7_gammaq(0.5 * (double)k, 0.5 * H);
        }
    }
    double *st = a.state + (size_t)g * k19_state_stride(kc), *rs = a.rstate + (size_t)g * k16_state_stride(k);
    if (lane == 0) {
        st[0] = n; st[1] = ok ? 1.0 : 0.0; st[2] = n - (double)kc; st[3] = rsst;
        rs[1] = ok ? 1.0 : 0.0;
        if (a.status) a.status[g] = !(n > 0.0) ? POLS_GROUP_EMPTY : (!(dfw > 0.0 && dfb > 0.0) ? POLS_GROUP_BAD_DOF : (ok ? POLS_GROUP_OK : POLS_GROUP_FALLBACK));
        if (a.sigma2_e_out) a.sigma2_e_out[g] = ok ? s2e : q;
        if (a.sigma2_u) a.sigma2_u[g] = ok ? s2u : q;
        if (a.rho) a.rho[g] = ok ? s2u / (s2u + s2e) : q;
        if (a.hausman) a.hausman[g] = H;
        if (a.hausman_p) a.hausman_p[g] = Hp;
    }
    if (lane < kc) {
        const double b = ok ? rhs[lane] : q;
        st[8 + lane] = b;
        if (lane < k) rs[8 + lane] = b;
        fit_store_coef(a, g, kc, lane, ok ? b : (n > 0.0 ? q : 0.0));   // no rows: zeros, as the existing entries
        if (a.coef_between) a.coef_between[(size_t)g * kc + lane] = ok ? bb[lane] : q;
        if (lane < k && a.coef_within) a.coef_within[(size_t)g * k + lane] = ok ? ws[8 + lane] : q;
    }
    for (int p = lane; p < kc * kc; p += 64) st[8 + kc + p] = ok ? Minv[p] : q;
}

int k19_table_launch(pols_ctx *ctx, const RandomEffectsArgs &a, const bool resident, const int64_t grid) {
    if (grid == 0) return POLS_OK;
    const size_t lds = sizeof(double) * (size_t)k19_lds(a.k_user, a.kt, resident ? a.res_rows : 0).total;
    if (lds > FIT_LDS_BUDGET) return fail(POLS_ERR_UNSUPPORTED, "random_effects: %d table rows exceed the LDS of a workgroup", a.res_rows);
    static OncePerDevice once_res, once_glb;
    return resident ? fit_launch(ctx, &k19_table_kernel<true>, once_res, grid, 256, lds, FIT_LDS_BUDGET, a)
                    : fit_launch(ctx, &k19_table_kernel<false>, once_glb, grid, 256, lds, FIT_LDS_BUDGET, a);
}

// ---------------------------------------------------------------- finish
__global__ void __launch_bounds__(64) k19_finish_kernel(const RandomEffectsArgs a) {
    const int lane = threadIdx.x, kc = a.kt;
    const int64_t g = blockIdx.x;
    int64_t v0, v1;
    fit_group_items(a, g, v0, v1);
    const double *st = a.state + (size_t)g * k19_state_stride(kc);
    const double q = fit_nan();
    double se = q, tv = q, pv = q;
    if (st[1] != 0.0) {                                            // (wave-uniform)
        double l = 0.0;
        for (int64_t c = a.item_first[v0] + lane; c < a.item_first[v1]; c += 64) l += a.resid_part[c];
        const double rss = k16_wave_sum(l) + st[3], df = st[2], sigma2 = rss / df;
        if (lane < kc) fit_se_t_p(sigma2 * st[8 + kc + lane * kc + lane], st[8 + lane], df, se, tv, pv);
    }
    if (lane < kc) fit_store_stats(a, g, kc, lane, se, tv, pv);
}

int k19_finish_launch(pols_ctx *ctx, const RandomEffectsArgs &a) { return fit_launch_plain(ctx, k19_finish_kernel, a.n_groups, 64, 0, a); }

// ---------------------------------------------------------------- predict
template <typename T>
__global__ void __launch_bounds__(256) k19_predict_kernel(const RandomEffectsArgs a) {
    const int k = a.k_user, kc = a.kt;
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    if (e <= s) return;
    const double *st = a.state + (size_t)g * k19_state_stride(kc);
    T *const out[4] = {static_cast<T *>(a.pred), static_cast<T *>(a.resid), static_cast<T *>(a.effects), static_cast<T *>(a.theta)};
    fit_predict_rows<T>(a, s, e, base, st + 8, kc > k ? st[8 + k] : 0.0, (const T *)nullptr, out,
                        [&](const double lin, const double yv, const int64_t r, const bool in, const bool fit, double (&o)[4]) {
                            const double pr = fit ? lin : fit_nan();
                            o[0] = pr;
                            o[1] = yv - pr;
                            o[2] = in ? a.u_c[a.catidx[r]] : fit_nan();
                            o[3] = in ? a.theta_c[a.catidx[r]] : fit_nan();
                        });
}

int k19_predict_launch(pols_ctx *ctx, int dtype, const RandomEffectsArgs &a) {
    if (a.n_groups == 0 || a.n_rows == 0 || (!a.pred && !a.resid && !a.effects && !a.theta)) return POLS_OK;
    return dtype == POLS_F32 ? fit_launch_plain(ctx, k19_predict_kernel<float>, fit_items(a), 256, 0, a)
                             : fit_launch_plain(ctx, k19_predict_kernel<double>, fit_items(a), 256, 0, a);
}

}  // namespace pols
