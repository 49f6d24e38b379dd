// k16_absorb.hpp -- K16: per-group regression that absorbs one categorical effect, the "within" estimator (pols_least_squares_absorb).
#pragma once
#include "common.hpp"

namespace pols {

constexpr int K16_KMAX = 31;        // the frame's columns incl. the intercept (the one-wave solve: a lane per column)

// doubles per category of the table: fitted rows n_c (the solve launch puts the effect a_c there), W_c, ybar_c, xbar_c (k)
__host__ __device__ inline size_t k16_cat_stride(int k) { return 3 + (size_t)k; }
// doubles per item (segment / group) of the Gram launch: the packed upper triangle of [X~ | y~]'[X~ | y~], the k raw T_jj, the fitted rows
__host__ __device__ inline size_t k16_gram_stride(int k) { return (size_t)(k + 1) * (k + 2) / 2 + (size_t)k + 1; }
// doubles per group of the solve launch's state: n, usable (1 / 0), C, df, c0, sum y~^2, sum w (y - ybar_w)^2, sum W_c, then b (k), A^-1 (k x k)
__host__ __device__ inline size_t k16_state_stride(int k) { return 8 + (size_t)k + (size_t)k * k; }
// doubles per category of the residual launch: RSS_c, then (cluster) the k squares of z_c = A^-1 s_c
__host__ __device__ inline size_t k16_resid_stride(int k, bool cluster) { return 1 + (cluster ? (size_t)k : 0); }

struct AbsorbArgs {
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
    int32_t k_user, kt;          // k features and k + 1: fit_stage leaves sqrt(w) in column k of the tile (the fit itself has no ones column)
    int32_t icpt;                // add_intercept: coef[k] = c0 and fe = a_c - c0
    int32_t f32;                 // dtype of coef
    int32_t cluster;             // POLS_COV_CLUSTER
    const int64_t *ids;          // device, one per row
    const uint32_t *order;       // position -> row (k7c_order_launch), nullptr: the identity
    int32_t *item_cnt;           // items: the run starts inside the item                                    (Work::AbsorbIndex)
    int64_t *item_first;         // items + 1: their exclusive prefix = the first category that starts in the item; the total last
    int32_t *catidx;             // n_rows, frame order: the row's category
    int64_t *cat_start;          // n_cats + 1: the first position of every category, then the end of the frame (Work::AbsorbCats)
    int64_t n_cats;
    double *cat;                 // n_cats x k16_cat_stride
    double *resid_part;          // n_cats x k16_resid_stride
    double *gram_part;           // items x k16_gram_stride                                                  (Work::AbsorbMoments)
    double *state;               // n_groups x k16_state_stride
    // outputs, any may be nullptr
    void *coef;
    int32_t *status;
    void *pred, *resid, *fe;
    double *se, *t_values, *p_values, *sigma2, *r2_within, *r2;
    int64_t *n_obs, *n_categories;
};

// run starts per item, their prefix over the items (one workgroup); a.item_first[items] is the number of categories
int k16_count_launch(pols_ctx *ctx, const AbsorbArgs &a);
// the category of every row and the first position of every category
int k16_index_launch(pols_ctx *ctx, const AbsorbArgs &a);
// one wave per category: n_c, W_c and the weighted means of y and the k features
int k16_means_launch(pols_ctx *ctx, int dtype, const AbsorbArgs &a);
// one workgroup per segment / group: the moments of the demeaned rows, the raw second moments, the fitted rows
int k16_gram_launch(pols_ctx *ctx, int dtype, const AbsorbArgs &a);
// one wave per group: partials in segment order, Cholesky against the raw second moments, b, A^-1, the effects, c0, df, status
int k16_solve_launch(pols_ctx *ctx, const AbsorbArgs &a);
// one wave per category: RSS_c from the rows and (cluster) the squares of A^-1 s_c
int k16_resid_launch(pols_ctx *ctx, int dtype, const AbsorbArgs &a);
// one wave per group: RSS over the categories in ascending order, sigma2, se / t / p, r2_within, r2
int k16_finish_launch(pols_ctx *ctx, const AbsorbArgs &a);
// one workgroup per segment / group: pred, resid and fe of every row
int k16_predict_launch(pols_ctx *ctx, int dtype, const AbsorbArgs &a);

}  // namespace pols
