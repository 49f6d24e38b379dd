// k14_iv.hpp -- K14: two-stage least squares (instrumental variables) per group with first-stage and Sargan diagnostics (pols_iv2sls).
#pragma once
#include "common.hpp"

namespace pols {

constexpr int K14_TMAX = 31;        // regressors incl. the intercept plus excluded instruments (K10's cap: its Gram launch forms the moments)

// doubles per group of the solve launch's state: n, usable (1 / 0), the Sargan numerator |r - Q b|^2, one spare, then b (kx),
// M^-1 (kx x kx) and Pi (L x kx, rows in the order [X1 | Z2 | 1] of the staged tile)
__host__ __device__ inline size_t k14_state_stride(int kx, int L) { return 4 + (size_t)kx + (size_t)kx * kx + (size_t)L * kx; }
// doubles per item (segment / group) of the rows launch: RSS, then (robust) the packed upper triangle of sum e~^2 x^ x^'
__host__ __device__ inline size_t k14_rows_stride(int kx, bool robust) { return 1 + (robust ? (size_t)kx * (kx + 1) / 2 : 0); }

struct IvArgs {
    const void *y;
    const void *w;               // null weights already filled (fill_null_weights), or nullptr
    const void *x[POLS_MAX_FEATURES];   // the concatenated list [X1 | X2 | Z2]: what K10's Gram launch and fit_stage see as the features
    const int64_t *offs;         // DEVICE offsets of the frame's groups
    int64_t n_groups, n_rows;
    const int64_t *seg_offs;     // long groups cut into segments (ensure_segments) or nullptr: one workgroup per group
    const int32_t *seg_map, *seg_first;
    int64_t n_seg;
    const uint8_t *valid;        // optional, drop family only
    int32_t null_policy;
    int32_t k_user, kt;          // of the staged list: n_feat + n_inst columns, T = k_user + intercept (plain rows launch: n_feat, kx)
    int32_t n_feat, n_endog, n_inst, icpt;   // the regressors [X1 | X2] (the last n_endog endogenous), the excluded instruments, ones column
    int32_t f32;                 // dtype of coef
    int32_t cov_type, small_sample;
    int32_t pred_all;            // coefp is laid out for the concatenated list (zeros for Z2): "drop" masks the rows with a null instrument
    const double *gram_part;     // items x k10_gram_stride(T): K10's Gram launch over the concatenated list  (Work::IvMoments)
    double *rows_part;           // items x k14_rows_stride                                                  (Work::IvMoments, behind gram_part)
    double *state;               // n_groups x k14_state_stride                                              (Work::IvState)
    double *coefp;               // n_groups x (pred_all ? T : kx): the coefficients for the prediction pass (Work::IvState, behind state)
    // outputs, any may be nullptr
    void *coef;
    int32_t *status;
    double *se, *t_values, *p_values, *cov, *sigma2, *first_stage_f, *partial_r2, *sargan, *sargan_p;
    int64_t *n_obs;
};

// dynamic LDS of the solve launch's one wave (bytes): the summed moments, Z~'Z~ and its factor, [C | Z~'y~] -> [Q | r], the packed
// [M, Q'r], its factor and the inverse of that factor
size_t k14_solve_lds(int kx, int L, int T);
// one wave per group: moments summed in segment order, both factorisations, b, M^-1, Pi, first-stage diagnostics, Sargan numerator, status
int k14_solve_launch(pols_ctx *ctx, const IvArgs &a);
// one workgroup per segment / group: e~ from the actual regressors, RSS and (robust) the meat partials
int k14_rows_launch(pols_ctx *ctx, int dtype, const IvArgs &a);
// one wave per group: sigma2, V, se / t / p, Sargan and its p-value
int k14_finish_launch(pols_ctx *ctx, const IvArgs &a);

}  // namespace pols
