// k19_random_effects.hpp -- K19: per-group random-effects panel regression with the Hausman test (pols_random_effects).
#pragma once
#include "common.hpp"
#include "fit_lds.hpp"

namespace pols {

constexpr int K19_KMAX = 31;        // the frame's columns incl. the intercept (the one-wave solves: a lane per column)

// doubles per group of the table kernel's state: n, usable (1 / 0), df = n - kc, the table's part of RSS, four spare, then b (kc), M^-1 (kc x kc)
__host__ __device__ inline size_t k19_state_stride(int kc) { return 8 + (size_t)kc + (size_t)kc * kc; }

struct RandomEffectsArgs {
    const void *y;
    const void *w;               // always nullptr (weights are refused); fit_predict_rows' argument set
    const void *x[POLS_MAX_FEATURES];
    const int64_t *offs;         // DEVICE offsets of the frame's groups
    int64_t n_groups, n_rows;
    const int64_t *seg_offs;     // long groups cut into segments (ensure_segments) or nullptr
    const int32_t *seg_map, *seg_first;
    int64_t n_seg;
    const uint8_t *valid;
    int32_t null_policy;
    int32_t k_user, kt;          // k features; kt = kc = k + intercept
    int32_t f32;                 // dtype of coef
    int32_t res_rows;            // table rows the resident launch lays its LDS out for
    // K16's products (an AbsorbArgs of the same call)
    const int64_t *item_first;   // items + 1: the first category of every item
    const int32_t *catidx;       // n_rows: the row's category
    const double *cat;           // n_cats x k16_cat_stride: (a_c), T_c, ybar_c, xbar_c
    const double *gram_part;     // items x k16_gram_stride: the within moments
    const double *wstate;        // n_groups x k16_state_stride: n, usable, C, df_w, .., b_w, A_w^-1
    const double *sigma2_e;      // n_groups: RSS_w / df_w (K16's finish launch)
    const double *resid_part;    // n_cats: the row term of RSS per category (K16's resid launch with b)
    // K19's work
    const int32_t *list;         // the groups of this launch (a mixed frame) or nullptr: every group
    int64_t *table_rows;         // n_groups: the rows of the table per group, for the host's route split
    double *theta_c, *u_c, *q_c; // n_cats each
    double *state;               // n_groups x k19_state_stride
    double *rstate;              // n_groups x k16_state_stride: usable and b where K16's resid launch reads them
    // outputs, any may be nullptr
    void *coef;
    int32_t *status;
    void *pred, *resid, *effects, *theta;
    double *se, *t_values, *p_values, *coef_between, *coef_within, *sigma2_e_out, *sigma2_u, *rho, *hausman, *hausman_p;
};

// one thread per group: the rows of the category table the group spans
int k19_rows_launch(pols_ctx *ctx, const RandomEffectsArgs &a);
// one workgroup per group of the launch: between fit, variance components, GLS, effects, Hausman.  grid: groups of this launch.
int k19_table_launch(pols_ctx *ctx, const RandomEffectsArgs &a, bool resident, int64_t grid);
// one wave per group: RSS, sigma2, se / t / p
int k19_finish_launch(pols_ctx *ctx, const RandomEffectsArgs &a);
// one workgroup per segment / group: pred, resid, effects, theta of every row
int k19_predict_launch(pols_ctx *ctx, int dtype, const RandomEffectsArgs &a);

}  // namespace pols
