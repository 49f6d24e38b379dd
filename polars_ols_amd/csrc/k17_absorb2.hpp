// k17_absorb2.hpp -- K17: per-group regression that absorbs two categorical effects by alternating projections (pols_least_squares_absorb2).
#pragma once
#include "common.hpp"
#include "fit_launch.hpp"

namespace pols {

constexpr int K17_KMAX = 31;        // the frame's columns incl. the intercept (K16's one-wave solve: a lane per column)

// The resident store of one (group, column) workgroup of the demean launch, n rows: the column (f64), the weights (f64, only when the
// store carries them), perm2 (16 bit) and the two start tables (16 bit, C1 + 1 and C2 + 1 entries, laid out for the worst case
// C1 = C2 = n so that the host needs no per-group category count):  8 n [+ 8 n] + 2 n + 2 (n + 1) + 2 (n + 1) = 14 n + 4 | 22 n + 4 bytes.
__host__ __device__ inline size_t k17_resident_bytes(int64_t n, bool has_w) { return (size_t)n * (has_w ? 22 : 14) + 4; }
// ... and the longest group it takes: 11 684 rows without weights, 7 435 with (FIT_LDS_BUDGET = 163 584 bytes)
inline int64_t k17_resident_rows(bool has_w) { return (int64_t)((FIT_LDS_BUDGET - 4) / (has_w ? 22 : 14)); }

// doubles per (group, column) of the demean launch: T_jj = sum w v0^2, sum w (v0 - vbar_w)^2 (the target's only), sweeps made, stop rule fired (1 / 0)
constexpr size_t K17_COLSTAT = 4;
// doubles per group of the label workgroup: n, sum w, C1, C2, M
constexpr size_t K17_GRPSTAT = 8;
// doubles per item (segment / group) of the Gram launch: the packed upper triangle of [X~ | y~]'[X~ | y~]
__host__ __device__ inline size_t k17_gram_stride(int k) { return (size_t)(k + 1) * (k + 2) / 2; }
// doubles per group of the solve launch's state: n, usable (1 / 0), C1, df, c0, sum y~^2, sum w (y - ybar_w)^2, sum w, C2, M, the weighted
// means of a1 and of a2 over the fitted rows, four spare, then b (k), A^-1 (k x k)
__host__ __device__ inline size_t k17_state_stride(int k) { return 16 + (size_t)k + (size_t)k * k; }
// doubles per id-1 category of the residual launch: RSS_c, then (cluster) the k squares of z_c = A^-1 s_c
__host__ __device__ inline size_t k17_resid_stride(int k, bool cluster) { return 1 + (cluster ? (size_t)k : 0); }

struct Absorb2Args {
    const void *y;
    const void *w;               // null weights already filled (fill_null_weights), or nullptr
    const void *x[POLS_MAX_FEATURES];
    const int64_t *offs;         // DEVICE offsets of the frame's groups
    int64_t n_groups, n_rows;
    const int64_t *seg_offs;     // long groups cut into segments (ensure_segments) or nullptr: one workgroup per group
    const int32_t *seg_map, *seg_first;
    int64_t n_seg;
    const uint8_t *valid;        // optional, drop family only
    int32_t null_policy;
    int32_t k_user, kt;          // k features and k + 1 (the fit has no ones column)
    int32_t icpt;                // add_intercept: coef[k] = c0, fe1 / fe2 centred
    int32_t f32;                 // dtype of coef
    int32_t cluster;             // POLS_COV_CLUSTER
    int32_t has_w;               // the demean stores carry weights: a weights column, or a policy that can take rows out of the fit (weight 0)
    int32_t max_iter;
    double tol;
    // K7c's orders and K16's category tables of the two id columns (k16_count_launch / k16_index_launch)
    const uint32_t *order1, *order2;   // position -> row, nullptr: the identity
    const int64_t *first1, *first2;    // items + 1: the first category that starts in the item
    const int32_t *catidx1, *catidx2;  // n_rows, frame order: the row's category
    const int64_t *start1, *start2;    // n_cats + 1: the first position of every category, then the end of the frame
    int64_t n_cats1, n_cats2;
    uint32_t *pos1;              // n_rows: row -> id-1 position                                               (Work::Absorb2Order)
    uint32_t *perm2;             // n_rows: id-2 position -> id-1 position, LOCAL to the group
    double *cols;                // (k + 1) x n_rows, id-1 order: v0, then the demeaned columns (y last)       (Work::Absorb2Cols)
    double *wfit;                // n_rows, id-1 order: the weight of a fitted row (1 without weights), 0 outside the fit
    int32_t *rowlab;             // n_rows, id-1 order: the component labels of the rows while they are propagated
    uint8_t *fitb;               // n_rows, id-1 order: the row is fitted
    double *am1, *am2;           // (k + 1) x n_cats: the accumulated means a1(v), a2(v)                       (Work::Absorb2Cats)
    double *aw1, *aw2;           // (k + 1) x n_cats: W_c as the workgroup of each column summed it (only when has_w)
    double *wc1, *wc2;           // n_cats: W_c (the label workgroup's, for the solve launch)
    double *eff1, *eff2;         // n_cats: the effects a1_c, a2_d (NaN: no fitted row, or no fit)
    int32_t *lab1, *lab2;        // n_cats: the component (its smallest id-1 category, local), -1 without a fitted row
    double *resid_part;          // n_cats1 x k17_resid_stride
    double *colstat;             // n_groups x (k + 1) x K17_COLSTAT                                           (Work::Absorb2Moments)
    double *grpstat;             // n_groups x K17_GRPSTAT
    double *gram_part;           // items x k17_gram_stride
    double *state;               // n_groups x k17_state_stride
    const int32_t *list;         // the groups of this demean launch (a frame that needs both routes), or nullptr: every group
    int64_t n_list;
    // outputs, any may be nullptr
    void *coef;
    int32_t *status;
    void *pred, *resid, *fe1, *fe2;
    double *se, *t_values, *p_values, *sigma2, *r2_within, *r2;
    int64_t *n_obs, *n_categories, *n_categories2, *n_components;
    int32_t *n_iter;
};

// one thread per id-1 position: the row's values as the fit sees them into cols / wfit / fitb, and pos1; then perm2
int k17_stage_launch(pols_ctx *ctx, int dtype, const Absorb2Args &a);
// one workgroup per (group, column) and one per group for the component labels; resident: the column store is LDS (a.list / a.n_list:
// the groups that fit), else the global scratch itself.  max_rows: the longest group of the launch.
int k17_demean_launch(pols_ctx *ctx, const Absorb2Args &a, bool resident, int64_t max_rows);
// one workgroup per segment / group: the moments of the demeaned columns
int k17_gram_launch(pols_ctx *ctx, const Absorb2Args &a);
// one wave per group: df, K16's solve, the effects, c0, status, the counts
int k17_solve_launch(pols_ctx *ctx, const Absorb2Args &a);
// one wave per id-1 category: RSS_c and (cluster) the squares of A^-1 s_c
int k17_resid_launch(pols_ctx *ctx, const Absorb2Args &a);
// one wave per group: RSS over the categories in ascending order, sigma2, se / t / p, r2_within, r2
int k17_finish_launch(pols_ctx *ctx, const Absorb2Args &a);
// one workgroup per segment / group: pred, resid, fe1 and fe2 of every row
int k17_predict_launch(pols_ctx *ctx, int dtype, const Absorb2Args &a);

}  // namespace pols
