// k18_glsar.hpp -- K18: AR(1) feasible GLS per group, Cochrane-Orcutt / Prais-Winsten (pols_glsar).
#pragma once
#include "common.hpp"

namespace pols {

constexpr int K18_KMAX = 31;        // columns incl. the intercept (the family's cap); T = kt + 1 staged columns with y

// doubles per item (segment / group) of the lag-Gram launch: the packed upper triangle of S = sum z z', the full T x T lag-one
// cross-moments C = sum z_t z_{t-1}' (row i: z_t's column, column j: z_{t-1}'s), then the item's fitted rows
__host__ __device__ inline size_t k18_gram_stride(int kt) { return (size_t)(kt + 1) * (kt + 2) / 2 + (size_t)(kt + 1) * (kt + 1) + 1; }
// doubles per group of the solve launch's state: n, usable (1 / 0), rho*, sqrt(1 - rho*^2), then b (kt), b0 (kt), A_xx(rho*)^-1 (kt x kt)
__host__ __device__ inline size_t k18_state_stride(int kt) { return 4 + 2 * (size_t)kt + (size_t)kt * kt; }
// doubles per item of the rows launch: RSS*, sum (u_t - u_{t-1})^2, sum (e0_t - e0_{t-1})^2, sum e0_t^2
constexpr size_t K18_ROWS_STRIDE = 4;

struct GlsarArgs {
    const void *y;
    const void *w;               // always nullptr: weights are not built (fit_stage reads the field)
    const void *x[POLS_MAX_FEATURES];
    const int64_t *offs;         // DEVICE offsets of the frame's groups
    int64_t n_groups, n_rows;
    const int64_t *seg_offs;     // long groups cut into segments (ensure_segments) or nullptr: one workgroup per group
    const int32_t *seg_map, *seg_first;
    int64_t n_seg;
    const uint8_t *valid;        // always nullptr: the drop family is not built
    int32_t null_policy;         // POLS_NULL_IGNORE or POLS_NULL_ZERO: every row is a fitted row
    int32_t k_user, kt;
    int32_t f32;                 // dtype of coef
    int32_t method, max_iter;    // POLS_AR1_*
    double tol;
    double *gram_part;           // items x k18_gram_stride(kt)                                         (Work::GlsarMoments)
    double *rows_part;           // items x K18_ROWS_STRIDE                                             (Work::GlsarMoments, behind gram_part)
    double *state;               // n_groups x k18_state_stride(kt)                                     (Work::GlsarState)
    double *coefp;               // n_groups x kt: the coefficients for the prediction pass             (Work::GlsarState, behind state)
    // outputs, any may be nullptr
    void *coef;
    int32_t *status;
    double *se, *t_values, *p_values, *cov, *sigma2, *rho, *dw, *dw_ols;
    int32_t *n_iter;
    int64_t *n_obs;
};

// dynamic LDS of the launches (bytes)
size_t k18_gram_lds(int kt);
size_t k18_solve_lds(int kt);
// one workgroup per segment / group: S, C and the row count of the item
int k18_gram_launch(pols_ctx *ctx, int dtype, const GlsarArgs &a);
// one wave per group: the partials summed in segment order, z_1 and z_n, the whole iteration, b, b0, rho*, A_xx^-1, n_iter, status, coef
int k18_solve_launch(pols_ctx *ctx, int dtype, const GlsarArgs &a);
// one workgroup per segment / group: e and e0 per row, the partials of RSS*, sum (du)^2, sum (de0)^2, sum e0^2
int k18_rows_launch(pols_ctx *ctx, int dtype, const GlsarArgs &a);
// one wave per group: sigma2, V, se / t / p, dw, dw_ols
int k18_finish_launch(pols_ctx *ctx, const GlsarArgs &a);

}  // namespace pols
