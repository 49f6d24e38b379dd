// k17_absorb2.hip -- K17: per-group regression that absorbs two categorical effects (pols_least_squares_absorb2): the two-way within
// transform by alternating projections, then K16's solve on the demeaned columns.  The definitions are in include/pols_mi355x.h.
//
// Per group g the rows are kept in id-1 order (K7c's order of `ids`): a category of id 1 is a run of positions, a category of id 2 is a
// run of positions of the id-2 order, reached through perm2 (id-2 position -> id-1 position, local to the group).  Rows outside the fit
// stay in the stores with weight 0 and value 0.  Everything is f64; no atomics; every sum in a fixed order.
//
// Launches (behind K7c's order builder and K16's count / scan / index launches on each id column):
//   stage    one thread per id-1 position: the row's k + 1 values as the policy leaves them into the column scratch (k + 1) x n_rows,
//            its weight (0 outside the fit), its fit byte, and row -> position; a second launch turns that into perm2.
//   demean   grid G x (k + 2), 256 threads.  Workgroup (g, j <= k) owns column j of group g for the whole iteration: it loads the column
//            (and w, perm2, the start tables) into its store once, sweeps until the stop rule fires or max_iter, and writes the column back.
//            A half-sweep hands category c to wave c mod 4: the wave walks the category's positions in batches of 64 that meet in the
//            DPP tree of k16_wave_sum, the batches added in position order -- the order does not depend on which wave took the category
//            -- then subtracts the mean from the same positions; lane 0 adds the mean to the accumulated-means table (read at the head
//            of the category).  W_c is summed once per workgroup, in the same batches, into a table beside it.  max |m| of the
//            sweep is reduced over the four waves through LDS and every wave takes the same decision.  The sweep is written once over
//            a store: ResidentStore (LDS, 16-bit perm2 / starts; groups up to k17_resident_rows) and GlobalStore (the scratch itself,
//            any length); the same code in the same order, so a group gives the same bits on either.
//            Workgroup (g, k + 1) propagates int32 labels over the same two families of runs with min in the place of mean until
//            nothing changes: the component of every category, M, and n, sum w, W_c, C1, C2 of the group.
//   gram     per item (segment / group), id-1 order: 256-position tiles of sqrt(w) x the demeaned columns, TriSpread accumulation.
//   solve    one wave per group: partials in segment order, df = n - k - (C1 + C2 - M), k16_solve_core against the T_jj of the demean
//            launch, the effects a1_c / a2_d from the accumulated means, their weighted means, c0, status, counts.
//   resid    one wave per id-1 category: e~ from the demeaned columns, RSS_c, (cluster) z = A^-1 s_c.
//   finish   one wave per group: RSS, sigma2, se / t / p, r2_within, r2 (absorb_finish, K16's).
//   predict  per item, fit_predict_rows: pred = x'b + a1 + a2 where the row's two categories lie in one component.
#include "k17_absorb2.hpp"
#include "k16_absorb.inl"

#include <algorithm>

namespace pols {

constexpr int K17_NOLABEL = 0x7fffffff;

// the first and one-past-last category of group g in a table of k16_count_launch
__device__ __forceinline__ void k17_cats(const Absorb2Args &a, const int64_t *first, const int64_t g, int64_t &c0, int64_t &c1) {
    int64_t v0, v1;
    fit_group_items(a, g, v0, v1);
    c0 = first[v0];
    c1 = first[v1];
}
// max that keeps a NaN once it has one
__device__ __forceinline__ double k17_nanmax(const double a, const double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ int k17_wave_min(int v) {
    for (int off = 32; off; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}
// the sum of v over the 256 threads in every thread; red: four ints.  Two barriers.
__device__ __forceinline__ int k17_block_sum_int(int v, int *red, const int lane, const int wv) {
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[wv] = v;
    __syncthreads();
    const int r = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------- stage
template <typename T>
__global__ void __launch_bounds__(256) k17_stage_kernel(const Absorb2Args a) {
    __shared__ const void *xp[POLS_MAX_FEATURES];
    const int tid = threadIdx.x, k = a.k_user, pol = a.null_policy;
    k16_columns(a, xp, tid);
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 256 + tid, N = a.n_rows;
    if (p >= N) return;
    const int64_t r = a.order1 ? (int64_t)a.order1[p] : p;
    const bool fit = null_row_in_fit<T>(pol, a.valid, a.y, xp, k, r);
    const T *wp = static_cast<const T *>(a.w);
    a.pos1[r] = (uint32_t)p;
    a.fitb[p] = fit ? 1 : 0;
    a.wfit[p] = !fit ? 0.0 : (wp ? (double)wp[r] : 1.0);
    for (int j = 0; j < k; ++j) a.cols[(size_t)j * N + p] = fit ? (double)null_fill<T>(pol, static_cast<const T *>(xp[j])[r]) : 0.0;
    a.cols[(size_t)k * N + p] = fit ? (double)null_fill<T>(pol, static_cast<const T *>(a.y)[r]) : 0.0;
}

__global__ void __launch_bounds__(256) k17_perm_kernel(const Absorb2Args a) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.n_rows) return;
    const int64_t r = a.order2 ? (int64_t)a.order2[q] : q;
    const int64_t g = k16_group_of(a.offs, a.n_groups, q);
    a.perm2[q] = (uint32_t)((int64_t)a.pos1[r] - a.offs[g]);
}

int k17_stage_launch(pols_ctx *ctx, int dtype, const Absorb2Args &a) {
    if (a.n_rows == 0) return POLS_OK;
    const unsigned nb = (unsigned)((a.n_rows + 255) / 256);
    if (dtype == POLS_F32) hipLaunchKernelGGL(k17_stage_kernel<float>, dim3(nb), dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(k17_stage_kernel<double>, dim3(nb), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k17_perm_kernel, dim3(nb), dim3(256), 0, ctx->stream, a);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

// ---------------------------------------------------------------- demean
// The column store of one workgroup: positions are local to the group, 0 .. n.
struct ResidentStore {
    double *v;
    const double *w;
    const uint16_t *pm, *s1, *s2;
    __device__ __forceinline__ double get(const int p) const { return v[p]; }
    __device__ __forceinline__ void put(const int p, const double x) const { v[p] = x; }
    __device__ __forceinline__ double wt(const int p) const { return w[p]; }
    __device__ __forceinline__ int perm(const int q) const { return pm[q]; }
    __device__ __forceinline__ int start1(const int c) const { return s1[c]; }
    __device__ __forceinline__ int start2(const int c) const { return s2[c]; }
};
struct GlobalStore {
    double *v;
    const double *w;
    const uint32_t *pm;
    const int64_t *s1, *s2;      // the group's slices of the frame's start tables (frame positions)
    int64_t gs;
    __device__ __forceinline__ double get(const int p) const { return v[p]; }
    __device__ __forceinline__ void put(const int p, const double x) const { v[p] = x; }
    __device__ __forceinline__ double wt(const int p) const { return w[p]; }
    __device__ __forceinline__ int perm(const int q) const { return (int)pm[q]; }
    __device__ __forceinline__ int start1(const int c) const { return (int)(s1[c] - gs); }
    __device__ __forceinline__ int start2(const int c) const { return (int)(s2[c] - gs); }
};

// W_c of the ncat categories of id 1 (SECOND: of id 2) into aw, once per workgroup: the batches and the tree of the half-sweeps
template <bool SECOND, typename S>
__device__ __forceinline__ void k17_cat_weights(const S &st, const int ncat, double *aw, const int lane, const int wv) {
    for (int c = wv; c < ncat; c += 4) {
        const int p0 = SECOND ? st.start2(c) : st.start1(c), p1 = SECOND ? st.start2(c + 1) : st.start1(c + 1);
        double sw = 0.0;
        for (int pb = p0; pb < p1; pb += 64) {
            const int q = pb + lane;
            const bool live = q < p1;
            const int p = !live ? 0 : (SECOND ? st.perm(q) : q);
            sw = __dadd_rn(sw, k16_wave_sum(!live ? 0.0 : st.wt(p)));
        }
        if (lane == 0) aw[c] = sw;
    }
}

// One half-sweep over the ncat categories of id 1 (SECOND: of id 2, through perm2): wave wv takes categories wv, wv + 4, ..; returns
// the largest |m| among them.  am: the accumulated means of this column, one per category; aw: W_c (HASW; else the run length).  Both
// are read at the head of a category, so that the trip to the table is behind the category's sums when its value is needed.  All 64
// lanes of every wave stay active.
template <bool SECOND, bool HASW, typename S>
__device__ __forceinline__ double k17_half_sweep(const S &st, const int ncat, double *am, const double *aw, const int lane, const int wv) {
    double mx = 0.0;
    for (int c = wv; c < ncat; c += 4) {
        const int p0 = SECOND ? st.start2(c) : st.start1(c), p1 = SECOND ? st.start2(c + 1) : st.start1(c + 1);
        const double prev = am[c];
        const double sw = HASW ? aw[c] : (double)(p1 - p0);
        double sv = 0.0;
        for (int pb = p0; pb < p1; pb += 64) {
            const int q = pb + lane;
            const bool live = q < p1;
            const int p = !live ? 0 : (SECOND ? st.perm(q) : q);
            const double vi = !live ? 0.0 : st.get(p);
            const double t = HASW ? __dmul_rn(!live ? 0.0 : st.wt(p), vi) : vi;
            sv = __dadd_rn(sv, k16_wave_sum(t));
        }
        const double m = sw > 0.0 ? sv / sw : 0.0;                 // (a category without a fitted row: nothing to take out)
        for (int pb = p0; pb < p1; pb += 64) {
            const int q = pb + lane;
            if (q < p1) {
                const int p = SECOND ? st.perm(q) : q;
                st.put(p, __dsub_rn(st.get(p), m));
            }
        }
        if (lane == 0) am[c] = __dadd_rn(prev, m);
        mx = k17_nanmax(mx, fabs(m));
    }
    return mx;
}

// the workgroup of column j: statistics of v0, the iteration, the column's record.  red: four doubles of LDS.
template <bool HASW, typename S>
__device__ __forceinline__ void k17_iterate(const Absorb2Args &a, const S &st, const int n, const int C1, const int C2, double *am1, double *am2,
                                            double *aw1, double *aw2, double *rec, const bool target, double *red) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // sum w, sum w v0, sum w v0^2 (= T_jj): a thread takes positions tid, tid + 256, .., the threads meet in fit_block_sum
    double lw = 0.0, lv = 0.0, lq = 0.0;
    for (int p = tid; p < n; p += 256) {
        const double wi = HASW ? st.wt(p) : 1.0, vi = st.get(p), t = __dmul_rn(wi, vi);
        lw = __dadd_rn(lw, wi);
        lv = __dadd_rn(lv, t);
        lq = fma(t, vi, lq);
    }
    const double W = fit_block_sum(lw, red, lane, wv), V = fit_block_sum(lv, red, lane, wv), T = fit_block_sum(lq, red, lane, wv);
    double tss = 0.0;
    if (target) {                                                  // (workgroup-uniform)
        const double mean = V / W;
        double lt = 0.0;
        for (int p = tid; p < n; p += 256) {
            const double wi = HASW ? st.wt(p) : 1.0, d = __dsub_rn(st.get(p), mean);
            lt = fma(__dmul_rn(wi, d), d, lt);
        }
        tss = fit_block_sum(lt, red, lane, wv);
    }
    if (HASW) {                                                    // W_c never changes: summed once, read by every sweep
        k17_cat_weights<false>(st, C1, aw1, lane, wv);
        k17_cat_weights<true>(st, C2, aw2, lane, wv);
        __syncthreads();
    }
    const double thr = a.tol * sqrt(T / W);
    int it = 0;
    bool fired = !(W > 0.0);                                       // (no fitted row: nothing to sweep; workgroup-uniform)
    while (!fired) {
        const double m1 = k17_half_sweep<false, HASW>(st, C1, am1, aw1, lane, wv);
        __syncthreads();
        const double m2 = k17_half_sweep<true, HASW>(st, C2, am2, aw2, lane, wv);
        if (lane == 0) red[wv] = k17_nanmax(m1, m2);
        __syncthreads();                                           // (red is written again behind the barrier between the next two halves)
        const double mx = k17_nanmax(k17_nanmax(red[0], red[1]), k17_nanmax(red[2], red[3]));
        ++it;
        if (mx <= thr || !(mx <= FIT_DBL_MAX)) { fired = true; break; }   // (not finite: the moments fail the group)
        if (it >= a.max_iter) break;
    }
    __syncthreads();
    if (tid == 0) { rec[0] = T; rec[1] = tss; rec[2] = (double)it; rec[3] = fired ? 1.0 : 0.0; }
}

// the label workgroup of group g (global memory throughout): components, M, n, sum w, W_c, C1, C2
__device__ __forceinline__ void k17_labels(const Absorb2Args &a, const int64_t g, const int64_t gs, const int n, const int64_t c1lo, const int C1,
                                           const int64_t c2lo, const int C2, double *red, int *ired) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int32_t *lab = a.rowlab + gs;
    const uint8_t *fb = a.fitb + gs;
    const double *wf = a.wfit + gs;
    const uint32_t *pm = a.perm2 + gs;
    const int64_t *s1 = a.start1 + c1lo, *s2 = a.start2 + c2lo;
    int lf = 0;
    double lw = 0.0;
    for (int p = tid; p < n; p += 256) {
        const bool fit = fb[p] != 0;
        const int64_t r = a.order1 ? (int64_t)a.order1[gs + p] : gs + p;
        lab[p] = fit ? (int32_t)((int64_t)a.catidx1[r] - c1lo) : K17_NOLABEL;
        lf += fit ? 1 : 0;
        lw = __dadd_rn(lw, wf[p]);
    }
    const int nfit = k17_block_sum_int(lf, ired, lane, wv);        // (its barriers publish lab)
    const double W = fit_block_sum(lw, red, lane, wv);
    for (;;) {
        int changed = 0;
        for (int half = 0; half < 2; ++half) {
            const int ncat = half ? C2 : C1;
            const int64_t *ss = half ? s2 : s1;
            for (int c = wv; c < ncat; c += 4) {
                const int p0 = (int)(ss[c] - gs), p1 = (int)(ss[c + 1] - gs);
                int mn = K17_NOLABEL;
                for (int pb = p0; pb < p1; pb += 64) {
                    const int q = pb + lane;
                    const int l = q < p1 ? lab[half ? (int)pm[q] : q] : K17_NOLABEL;
                    mn = min(mn, k17_wave_min(l));
                }
                for (int pb = p0; pb < p1; pb += 64) {
                    const int q = pb + lane;
                    if (q < p1) {
                        const int p = half ? (int)pm[q] : q;
                        const int l = lab[p];
                        if (l != K17_NOLABEL && l != mn) { lab[p] = mn; changed = 1; }
                    }
                }
            }
            __syncthreads();
        }
        if (k17_block_sum_int(changed, ired, lane, wv) == 0) break;   // (the same sum in every thread)
    }
    // the categories' labels and weights; a batch of w meets in the same tree and the batches in the same order as in the half-sweeps
    int lc1 = 0, lc2 = 0, lm = 0;
    for (int half = 0; half < 2; ++half) {
        const int ncat = half ? C2 : C1;
        const int64_t *ss = half ? s2 : s1;
        int32_t *lo = (half ? a.lab2 + c2lo : a.lab1 + c1lo);
        double *wo = (half ? a.wc2 + c2lo : a.wc1 + c1lo);
        for (int c = wv; c < ncat; c += 4) {
            const int p0 = (int)(ss[c] - gs), p1 = (int)(ss[c + 1] - gs);
            int mn = K17_NOLABEL;
            double sw = 0.0;
            for (int pb = p0; pb < p1; pb += 64) {
                const int q = pb + lane;
                const bool live = q < p1;
                const int p = !live ? 0 : (half ? (int)pm[q] : q);
                mn = min(mn, k17_wave_min(live ? lab[p] : K17_NOLABEL));
                sw = __dadd_rn(sw, k16_wave_sum(live ? wf[p] : 0.0));
            }
            if (lane == 0) {
                lo[c] = mn == K17_NOLABEL ? -1 : mn;
                wo[c] = sw;
                if (mn != K17_NOLABEL) { if (half) ++lc2; else { ++lc1; lm += mn == c ? 1 : 0; } }
            }
        }
    }
    const int C1f = k17_block_sum_int(lc1, ired, lane, wv), C2f = k17_block_sum_int(lc2, ired, lane, wv), M = k17_block_sum_int(lm, ired, lane, wv);
    if (tid == 0) {
        double *gr = a.grpstat + (size_t)g * K17_GRPSTAT;
        gr[0] = (double)nfit; gr[1] = W; gr[2] = (double)C1f; gr[3] = (double)C2f; gr[4] = (double)M;
    }
}

template <bool RESIDENT, bool HASW>
__global__ void __launch_bounds__(256) k17_demean_kernel(const Absorb2Args a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    __shared__ double red[4];
    __shared__ int ired[4];
    const int tid = threadIdx.x, k = a.k_user, per = k + 2;
    const int64_t li = blockIdx.x / per;
    const int j = (int)(blockIdx.x - li * per);
    const int64_t g = a.list ? (int64_t)a.list[li] : li;
    const int64_t gs = a.offs[g], N = a.n_rows;
    const int n = (int)(a.offs[g + 1] - gs);
    int64_t c1lo, c1hi, c2lo, c2hi;
    k17_cats(a, a.first1, g, c1lo, c1hi);
    k17_cats(a, a.first2, g, c2lo, c2hi);
    const int C1 = n > 0 ? (int)(c1hi - c1lo) : 0, C2 = n > 0 ? (int)(c2hi - c2lo) : 0;
    if (j == k + 1) {
        if (n == 0) {
            if (tid < 5) a.grpstat[(size_t)g * K17_GRPSTAT + tid] = 0.0;
            return;
        }
        k17_labels(a, g, gs, n, c1lo, C1, c2lo, C2, red, ired);
        return;
    }
    double *rec = a.colstat + ((size_t)g * (k + 1) + j) * K17_COLSTAT;
    if (n == 0) {
        if (tid < 4) rec[tid] = tid == 3 ? 1.0 : 0.0;
        return;
    }
    double *am1 = a.am1 + (size_t)j * a.n_cats1 + c1lo, *am2 = a.am2 + (size_t)j * a.n_cats2 + c2lo;
    double *aw1 = a.aw1 + (size_t)j * a.n_cats1 + c1lo, *aw2 = a.aw2 + (size_t)j * a.n_cats2 + c2lo;
    for (int c = tid; c < C1; c += 256) am1[c] = 0.0;
    for (int c = tid; c < C2; c += 256) am2[c] = 0.0;
    double *col = a.cols + (size_t)j * N + gs;
    if constexpr (RESIDENT) {
        double *v = dyn, *w = dyn + n;
        uint16_t *pm = reinterpret_cast<uint16_t *>(dyn + (HASW ? 2 * (size_t)n : (size_t)n)), *s1 = pm + n, *s2 = s1 + n + 1;
        for (int p = tid; p < n; p += 256) {
            v[p] = col[p];
            if (HASW) w[p] = a.wfit[gs + p];
            pm[p] = (uint16_t)a.perm2[gs + p];
        }
        for (int c = tid; c <= C1; c += 256) s1[c] = (uint16_t)(a.start1[c1lo + c] - gs);
        for (int c = tid; c <= C2; c += 256) s2[c] = (uint16_t)(a.start2[c2lo + c] - gs);
        __syncthreads();
        const ResidentStore st{v, w, pm, s1, s2};
        k17_iterate<HASW>(a, st, n, C1, C2, am1, am2, aw1, aw2, rec, j == k, red);
        for (int p = tid; p < n; p += 256) col[p] = v[p];          // (k17_iterate ends on a barrier)
    } else {
        __syncthreads();
        const GlobalStore st{col, a.wfit + gs, a.perm2 + gs, a.start1 + c1lo, a.start2 + c2lo, gs};
        k17_iterate<HASW>(a, st, n, C1, C2, am1, am2, aw1, aw2, rec, j == k, red);
    }
}

int k17_demean_launch(pols_ctx *ctx, const Absorb2Args &a, bool resident, int64_t max_rows) {
    const int64_t groups = a.list ? a.n_list : a.n_groups;
    if (groups == 0) return POLS_OK;
    const int64_t grid = groups * (a.k_user + 2);
    const bool hw = a.has_w != 0;
    if (!resident)
        return hw ? fit_launch_plain(ctx, k17_demean_kernel<false, true>, grid, 256, 0, a) : fit_launch_plain(ctx, k17_demean_kernel<false, false>, grid, 256, 0, a);
    if (max_rows > k17_resident_rows(hw)) return fail(POLS_ERR_INVALID, "absorb2: %lld rows do not fit the resident store", (long long)max_rows);
    const size_t lds = (k17_resident_bytes(max_rows, hw) + 15) & ~(size_t)15;
    static OncePerDevice once_w, once_u;
    return hw ? fit_launch(ctx, &k17_demean_kernel<true, true>, once_w, grid, 256, lds, FIT_LDS_BUDGET, a)
              : fit_launch(ctx, &k17_demean_kernel<true, false>, once_u, grid, 256, lds, FIT_LDS_BUDGET, a);
}

// ---------------------------------------------------------------- gram
__global__ void __launch_bounds__(256) k17_gram_kernel(const Absorb2Args a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int tid = threadIdx.x, k = a.k_user, nz = k + 1;
    constexpr int ts = FIT_TS;
    double *xs = dyn;                                              // (k + 1) x ts: x~, y~
    double *gp = xs + (size_t)nz * ts;                             // 256
    const int64_t sgi = blockIdx.x, N = a.n_rows;
    const int64_t g = a.seg_offs ? (int64_t)a.seg_map[sgi] : sgi;
    const int64_t s = a.seg_offs ? a.seg_offs[sgi] : a.offs[g], e = a.seg_offs ? a.seg_offs[sgi + 1] : a.offs[g + 1];
    const TriSpread sp = tri_spread(nz, tid);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t t0 = s; t0 < e; t0 += FIT_TILE) {
        const int64_t p = t0 + tid;
        const bool live = p < e;
        const double sw = live ? sqrt(a.wfit[p]) : 0.0;
        for (int c = 0; c < nz; ++c) xs[(size_t)c * ts + tid] = live ? sw * a.cols[(size_t)c * N + p] : 0.0;
        __syncthreads();
        tri_accumulate(sp, acc, xs, ts, 0, (int)min((int64_t)FIT_TILE, e - t0));
        __syncthreads();                                           // the next tile overwrites xs
    }
    tri_reduce(sp, acc, gp, a.gram_part + (size_t)blockIdx.x * k17_gram_stride(k));
}

int k17_gram_launch(pols_ctx *ctx, const Absorb2Args &a) {
    const int64_t items = fit_items(a);
    if (items == 0) return POLS_OK;
    const size_t lds = sizeof(double) * ((size_t)(a.k_user + 1) * FIT_TS + 256);
    static OncePerDevice once;
    return fit_launch(ctx, &k17_gram_kernel, once, items, 256, lds, FIT_LDS_BUDGET, a);
}

// ---------------------------------------------------------------- solve
__global__ void __launch_bounds__(64) k17_solve_kernel(const Absorb2Args a) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int lane = threadIdx.x, k = a.k_user, nz = k + 1, ne = nz * (nz + 1) / 2, kc = k + a.icpt;
    const AbsorbLds o = k17_lds(k);
    double *Gs = dyn + o.Gs, *Tl = dyn + o.T, *rhs = dyn + o.rhs;
    const int64_t g = blockIdx.x;
    int64_t v0, v1;
    fit_group_items(a, g, v0, v1);
    const double *gr = a.grpstat + (size_t)g * K17_GRPSTAT, *cr = a.colstat + (size_t)g * (k + 1) * K17_COLSTAT;
    const double n = gr[0], W = gr[1], C1 = gr[2], C2 = gr[3], M = gr[4];
    bool fin = fit_sum_parts(a.gram_part, k17_gram_stride(k), v0, v1, ne, Gs, lane);
    int sweeps = 0;
    bool fired = true;
    if (lane <= k) {
        const double t = cr[(size_t)lane * K17_COLSTAT];
        if (lane < k) Tl[lane] = t;
        fin = fin && fabs(t) <= FIT_DBL_MAX;
        sweeps = (int)cr[(size_t)lane * K17_COLSTAT + 2];
        fired = cr[(size_t)lane * K17_COLSTAT + 3] != 0.0;
    }
    const bool finite = __ballot(!fin) == 0, converged = __ballot(!fired) == 0;
    for (int off = 32; off; off >>= 1) sweeps = max(sweeps, __shfl_xor(sweeps, off));
    fit_wave_sync();
    const double yy = Gs[tri_index(k, k, nz)], tss = cr[(size_t)k * K17_COLSTAT + 1];
    const double df = n - (double)k - (C1 + C2 - M);
    bool ok = finite && n > 0.0 && df > 0.0;
    double *st = a.state + (size_t)g * k17_state_stride(k);
    ok = k16_solve_core(ok, dyn, o, st + 16 + k, k, lane);
    // the effects a1_c = a1_c(y) - sum_j b_j a1_c(x_j) into the tables (NaN for a category without a fitted row, and for a group without
    // a fit), and their weighted means over the fitted rows
    double mean[2];
    for (int half = 0; half < 2; ++half) {
        int64_t clo, chi;
        k17_cats(a, half ? a.first2 : a.first1, g, clo, chi);
        const int64_t nc = half ? a.n_cats2 : a.n_cats1;
        const double *am = half ? a.am2 : a.am1, *wc = half ? a.wc2 : a.wc1;
        const int32_t *lab = half ? a.lab2 : a.lab1;
        double *eff = half ? a.eff2 : a.eff1;
        double lA = 0.0;
        for (int64_t c = clo + lane; c < chi; c += 64) {
            double ac = fit_nan();
            if (ok && lab[c] >= 0) {
                ac = am[(size_t)k * nc + c];
                for (int j = 0; j < k; ++j) ac = fma(-am[(size_t)j * nc + c], rhs[j], ac);
                lA = fma(wc[c], ac, lA);
            }
            eff[c] = ac;
        }
        mean[half] = a.icpt ? k16_wave_sum(lA) / W : 0.0;
    }
    const double c0 = mean[0] + mean[1];
    if (lane == 0) {
        st[0] = n; st[1] = ok ? 1.0 : 0.0; st[2] = C1; st[3] = df; st[4] = ok ? c0 : fit_nan(); st[5] = yy; st[6] = tss; st[7] = W;
        st[8] = C2; st[9] = M; st[10] = ok ? mean[0] : fit_nan(); st[11] = ok ? mean[1] : fit_nan();
        if (a.status)
            a.status[g] = !(n > 0.0) ? POLS_GROUP_EMPTY
                          : (!(df > 0.0) ? POLS_GROUP_BAD_DOF : (!ok ? POLS_GROUP_FALLBACK : (!converged ? POLS_GROUP_NOT_CONVERGED : POLS_GROUP_OK)));
        if (a.n_obs) a.n_obs[g] = (int64_t)n;
        if (a.n_categories) a.n_categories[g] = (int64_t)C1;
        if (a.n_categories2) a.n_categories2[g] = (int64_t)C2;
        if (a.n_components) a.n_components[g] = (int64_t)M;
        if (a.n_iter) a.n_iter[g] = sweeps;
    }
    const double fillv = n > 0.0 ? fit_nan() : 0.0;                // no rows: zeros, as the existing entries
    if (lane < k) st[16 + lane] = ok ? rhs[lane] : fit_nan();
    if (lane < kc) fit_store_coef(a, g, kc, lane, ok ? (lane < k ? rhs[lane] : c0) : fillv);
}

int k17_solve_launch(pols_ctx *ctx, const Absorb2Args &a) {
    return fit_launch_plain(ctx, k17_solve_kernel, a.n_groups, 64, sizeof(double) * (size_t)k17_lds(a.k_user).total, a);
}

// ---------------------------------------------------------------- resid
__global__ void __launch_bounds__(64) k17_resid_kernel(const Absorb2Args a) {
    __shared__ double bs[K17_KMAX], ss[K17_KMAX], Ai[K17_KMAX * K17_KMAX];
    const int lane = threadIdx.x, k = a.k_user;
    const bool cluster = a.cluster != 0;
    const int64_t c = blockIdx.x, p0 = a.start1[c], p1 = a.start1[c + 1], N = a.n_rows;
    const int64_t g = k16_group_of(a.offs, a.n_groups, p0);
    const double *st = a.state + (size_t)g * k17_state_stride(k);
    double *out = a.resid_part + (size_t)c * k17_resid_stride(k, cluster);
    if (!absorb_resid_head(st, 16, 16 + k, out, cluster, k, lane, bs, Ai)) return;
    __syncthreads();
    double rss = 0.0, sacc = 0.0;                                  // sacc, lane j < k: s_cj
    for (int64_t pb = p0; pb < p1; pb += 64) {
        const int64_t p = pb + lane;
        const bool live = p < p1;
        double ev = 0.0, sw = 0.0;
        if (live) {
            sw = sqrt(a.wfit[p]);
            double f = a.cols[(size_t)k * N + p];
            for (int j = 0; j < k; ++j) f = fma(-a.cols[(size_t)j * N + p], bs[j], f);
            ev = sw * f;
        }
        rss = fma(ev, ev, rss);
        if (cluster) {
            for (int j = 0; j < k; ++j) {
                const double u = live ? ev * (sw * a.cols[(size_t)j * N + p]) : 0.0;
                const double t = k16_wave_sum(u);
                if (lane == j) sacc += t;
            }
        }
    }
    absorb_resid_tail(rss, sacc, ss, Ai, out, cluster, k, lane);
}

int k17_resid_launch(pols_ctx *ctx, const Absorb2Args &a) { return fit_launch_plain(ctx, k17_resid_kernel, a.n_cats1, 64, 0, a); }

// ---------------------------------------------------------------- finish
__global__ void __launch_bounds__(64) k17_finish_kernel(const Absorb2Args a) {
    const int k = a.k_user;
    const int64_t g = blockIdx.x;
    const double *st = a.state + (size_t)g * k17_state_stride(k);
    const double n = st[0], C1 = st[2], C2 = st[8], M = st[9];
    int64_t c0i, c1i;
    k17_cats(a, a.first1, g, c0i, c1i);
    const double d1 = n - (double)k - 1.0 - (C2 - M);              // the second effect is charged like regressors
    absorb_finish(a, g, st, c0i, c1i, k17_resid_stride(k, a.cluster != 0), C1, d1, 16, 16 + k);
}

int k17_finish_launch(pols_ctx *ctx, const Absorb2Args &a) { return fit_launch_plain(ctx, k17_finish_kernel, a.n_groups, 64, 0, a); }

// ---------------------------------------------------------------- predict
template <typename T>
__global__ void __launch_bounds__(256) k17_predict_kernel(const Absorb2Args a) {
    const int k = a.k_user;
    int64_t g, s, e, base, ntiles;
    fit_item<T>(a, g, s, e, base, ntiles);
    if (e <= s) return;
    const double *st = a.state + (size_t)g * k17_state_stride(k);
    const double m1 = st[10], m2 = st[11];
    int64_t c1lo, c1hi, c2lo, c2hi;
    k17_cats(a, a.first1, g, c1lo, c1hi);
    k17_cats(a, a.first2, g, c2lo, c2hi);
    T *const fe2 = static_cast<T *>(a.fe2);
    T *const out[3] = {static_cast<T *>(a.pred), static_cast<T *>(a.resid), static_cast<T *>(a.fe1)};
    fit_predict_rows<T>(a, s, e, base, st + 16, 0.0, (const T *)nullptr, out,
                        [&](const double lin, const double yv, const int64_t r, const bool in, const bool fit, double (&o)[3]) {
                            double a1 = fit_nan(), a2 = fit_nan();
                            if (in) {
                                const int64_t c = a.catidx1[r], d = a.catidx2[r];
                                const int l1 = a.lab1[c], l2 = a.lab2[d];
                                if (l1 >= 0 && l1 == l2) { a1 = a.eff1[c]; a2 = a.eff2[d]; }   // (a fitted row: always one component)
                            }
                            const double pr = lin + (a1 + a2);
                            o[0] = pr;
                            o[1] = yv - pr;
                            o[2] = a1 - m1;
                            if (in && fe2) fe2[r] = (T)(a2 - m2);
                        });
}

int k17_predict_launch(pols_ctx *ctx, int dtype, const Absorb2Args &a) {
    if (a.n_groups == 0 || a.n_rows == 0 || (!a.pred && !a.resid && !a.fe1 && !a.fe2)) return POLS_OK;
    return dtype == POLS_F32 ? fit_launch_plain(ctx, k17_predict_kernel<float>, fit_items(a), 256, 0, a)
                             : fit_launch_plain(ctx, k17_predict_kernel<double>, fit_items(a), 256, 0, a);
}

}  // namespace pols
