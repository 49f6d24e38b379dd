// k10_ridge_path.hpp -- K10: ridge regularisation path with closed-form leave-one-out selection (pols_ridge_cv).
#pragma once
#include "common.hpp"

namespace pols {

constexpr int K10_KMAX = 31;        // columns incl. the intercept (the K7 family's cap)
constexpr int K10_MAX_ALPHAS = 64;  // candidates of one call (one lane each in the pick launch)

// doubles per item (segment / group) of the Gram launch: the upper triangle of Z'Z, Z = [X~ | y~], then the item's fitted rows
__host__ __device__ inline size_t k10_gram_stride(int kt) { return (size_t)(kt + 1) * (kt + 2) / 2 + 1; }
// doubles per group of the eigen launch: V (kt x kt, row major: V[i * kt + m] = component i of eigenvector m), s, c = V'X~'y~, n
__host__ __device__ inline size_t k10_eig_stride(int kt) { return (size_t)kt * kt + 2 * (size_t)kt + 1; }

struct RidgeCvArgs {
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
    const double *alphas;        // DEVICE copy of the candidates
    int32_t n_alphas;
    double *gram_part;           // items x k10_gram_stride(kt)                                   (Work::RidgeCvGram)
    double *eig;                 // n_groups x k10_eig_stride(kt)                                 (Work::RidgeCvGram, behind gram_part)
    double *score_part;          // items x n_alphas                                              (Work::RidgeCvScores)
    double *coef64;              // n_groups x kt: the chosen coefficients for the prediction pass (Work::RidgeCvScores)
    // outputs, any may be nullptr
    double *alpha, *score, *cv_scores;
    int32_t *alpha_index, *status;
    void *coef, *coef_path;
    void *pred, *resid;          // n_rows, batch dtype, 16-byte aligned (the prediction launch)
};

int k10_gram_launch(pols_ctx *ctx, int dtype, const RidgeCvArgs &a);
int k10_eig_launch(pols_ctx *ctx, const RidgeCvArgs &a);
int k10_rows_launch(pols_ctx *ctx, int dtype, const RidgeCvArgs &a);
int k10_pick_launch(pols_ctx *ctx, const RidgeCvArgs &a);
int k10_predict_launch(pols_ctx *ctx, int dtype, const RidgeCvArgs &a);

}  // namespace pols
