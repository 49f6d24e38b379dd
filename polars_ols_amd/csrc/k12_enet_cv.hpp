// k12_enet_cv.hpp -- K12: elastic-net / lasso regularisation path with K-fold selection of alpha per group (pols_elastic_net_cv).
#pragma once
#include "common.hpp"
#include "k10_ridge_path.hpp"

namespace pols {

constexpr int K12_KMAX = 31;         // columns incl. the intercept (one lane each, 16 or 32 lanes per problem)
constexpr int K12_MAX_ALPHAS = 128;  // candidates of one call (one thread each in the pick launch)
constexpr int K12_MAX_FOLDS = 16;
constexpr int32_t K12_STOPPED = 1 << 30;   // flag on a sweep count: the fit ran into max_iter

struct EnetCvArgs {
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
    int32_t k_user, kt;
    int32_t f32;                 // dtype of coef / coef_path
    int32_t n_folds, n_alphas;
    int32_t automatic;           // the grid comes from the group's own X~'y~
    int32_t counted;             // the policy can remove rows: item_count holds every item's fitted rows
    int32_t max_iter, positive;
    double l1_ratio, tol, eps;
    const double *alphas;        // DEVICE copy of the explicit candidates                        (Work::EnetCvWork)
    const int32_t *order;        // candidate indices in visiting order: descending alpha, ties by index
    int64_t *item_count;         // items: fitted rows of a segment / group                       (Work::EnetCvGram)
    double *fold_part;           // items x n_folds x k10_gram_stride(kt)                         (Work::EnetCvGram)
    double *fold_gram;           // n_groups x n_folds x k10_gram_stride(kt): fold_part itself without segments
    double *score_part;          // n_groups x n_folds x n_alphas                                 (Work::EnetCvWork)
    int32_t *iters;              // n_groups x (n_folds + 1) x n_alphas: sweeps | K12_STOPPED
    double *path64;              // n_groups x n_alphas x kt: the full-data path in f64
    double *grid;                // n_groups x n_alphas: the candidates of every group
    double *coef64;              // n_groups x kt: the chosen coefficients for the prediction pass
    // outputs, any may be nullptr
    double *alpha, *score, *cv_scores, *alphas_used;
    int32_t *alpha_index, *n_iter, *status;
    void *coef, *coef_path;
};

int k12_count_launch(pols_ctx *ctx, int dtype, const EnetCvArgs &a);
int k12_fold_gram_launch(pols_ctx *ctx, int dtype, const EnetCvArgs &a);
int k12_reduce_launch(pols_ctx *ctx, const EnetCvArgs &a);
int k12_path_launch(pols_ctx *ctx, const EnetCvArgs &a);
int k12_pick_launch(pols_ctx *ctx, const EnetCvArgs &a);

}  // namespace pols
