// k7i_influence.hpp -- K7i: per-row influence diagnostics and prediction intervals (pols_least_squares_influence).
#pragma once
#include "k7r_robust.hpp"

namespace pols {

// per-row outputs, in the order of pols_influence_out's pointers
enum {
    K7I_LEVERAGE = 0, K7I_STUDENT_INT, K7I_STUDENT_EXT, K7I_COOKS_D, K7I_DFFITS, K7I_SE_MEAN, K7I_SE_OBS,
    K7I_MEAN_LO, K7I_MEAN_HI, K7I_OBS_LO, K7I_OBS_HI, K7I_NOUT
};

// the group stage: sigma2 / df / t_crit / usable of every group from K7's side-car RSS and K7r's prepare table
struct InflGroupArgs {
    const int64_t *offs;   // DEVICE offsets of the rows the fit ran on (the compacted frame under a null policy)
    int64_t n_groups;
    int32_t kt;
    double lambda, level;
    double *prep;          // n_groups x k7r_prep_stride(kt); with xe the refined coefficients replace b in it  (Work::InflPrep)
    const double *rss;     // n_groups                                                         (Work::InflGroup, first array)
    double *grp;           // 4 x n_groups: sigma2, df, t_crit, usable (ok and df > 0)          (Work::InflGroup, after rss)
    // f32 batches: one step of iterative refinement of b before anything is derived from it (k7i_refine_launch) -- or nullptr
    double *xe;                // (segments or groups) x kt: X~'e~ of the item's rows (overwritten) (Work::InflGroup, after grp)
    const int32_t *seg_first;  // group -> first segment, n_groups + 1, or nullptr: one item per group
};
int k7i_group_launch(pols_ctx *ctx, const InflGroupArgs &a);

// X~'e~ (e~ = y~ - X~ b, all in f64) of every segment / group into `xe`: a.s as K7 got it, a.prep the prepare table, a.part = xe
int k7i_refine_launch(pols_ctx *ctx, int dtype, const RobustArgs &a);

// the row pass: the ORIGINAL rows of the frame (valid == nullptr: every row was fitted)
struct InflArgs {
    const void *y;
    const void *w;
    const void *x[POLS_MAX_FEATURES];
    const int64_t *offs;       // DEVICE offsets of the frame's groups
    int64_t n_groups, n_rows;
    const int64_t *seg_offs;   // long groups cut into segments (ensure_segments) or nullptr: one workgroup per group
    const int32_t *seg_map;
    int64_t n_seg;
    const uint8_t *valid;      // the compaction's validity bytes (1 = the row was fitted) or nullptr; readable up to the next multiple of 16 rows
    int32_t zero_fill;         // with valid: the policy turns a null feature (and a fitted row's null target) into 0
    int32_t k_user, kt;
    const double *prep;        // as InflGroupArgs
    const double *grp;
    void *out[K7I_NOUT];       // n_rows each, batch dtype, 16-byte aligned, or nullptr
};
int k7i_rows_launch(pols_ctx *ctx, int dtype, const InflArgs &a);

}  // namespace pols
