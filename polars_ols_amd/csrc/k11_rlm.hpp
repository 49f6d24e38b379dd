// k11_rlm.hpp -- K11: Huber / bisquare M-estimator per group by iteratively reweighted least squares (pols_rlm).
#pragma once
#include "common.hpp"

namespace pols {

constexpr int K11_KMAX = 31;                          // columns incl. the intercept (K10's cap)
constexpr int64_t K11_STREAM_MAX_ROWS = (int64_t)1 << 22;   // rows of a group the streamed form takes (one workgroup walks them all)

struct RlmArgs {
    const void *y;
    const void *w;               // null weights already filled (fill_null_weights), or nullptr
    const void *x[POLS_MAX_FEATURES];
    const int64_t *offs;         // DEVICE offsets of the frame's groups
    int64_t n_groups, n_rows;
    const uint8_t *valid;        // optional, drop family only
    int32_t null_policy;
    int32_t k_user, kt;
    int32_t f32;                 // dtype of coef / weights
    int32_t norm, max_iter;
    double c, tol;
    int32_t res_tiles;           // the resident launch serves the groups of up to this many 256-row tiles, the streamed launch the others (-1: every group)
    int32_t ts;                  // resident launch: column stride of the LDS tile, 256 x (tiles of its longest group) + 1
    double *rows;                // n_rows: |r| / omega of the streamed groups' rows                  (Work::RlmRows)
    double *coef64;              // n_groups x kt: the coefficients for the prediction pass            (Work::RlmCoef)
    // outputs, any may be nullptr
    void *coef;
    int32_t *status;
    double *scale;
    int32_t *n_iter;
    void *weights;               // n_rows, batch dtype
};

// the most 256-row tiles of a group that stay resident in a workgroup's LDS at kt columns (0: none)
int k11_resident_tiles(int kt);
// one launch per form: resident for the groups of up to a.res_tiles tiles (skipped when a.res_tiles == 0), streamed for the others
int k11_rlm_launch(pols_ctx *ctx, int dtype, const RlmArgs &a, bool resident);

}  // namespace pols
