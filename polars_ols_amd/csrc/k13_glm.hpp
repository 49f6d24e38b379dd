// k13_glm.hpp -- K13: logistic / Poisson generalised linear model per group by iteratively reweighted least squares (pols_glm).
#pragma once
#include "common.hpp"

namespace pols {

constexpr int K13_KMAX = 31;                          // columns incl. the intercept (K10's cap)

// doubles per item (segment / group) of the split form's segment pass: the packed upper triangle of [X | z]' diag(W) [X | z], then the
// item's deviance part, fitted rows and rows outside the family's domain
__host__ __device__ inline size_t k13_part_stride(int kt) { return (size_t)(kt + 1) * (kt + 2) / 2 + 3; }
// doubles per group of the split form's state: iterating (1 / 0), the previous deviance, updates made, then b and se (kt each)
__host__ __device__ inline size_t k13_state_stride(int kt) { return 4 + 2 * (size_t)kt; }

struct GlmArgs {
    const void *y;
    const void *w;               // prior weights, null weights already filled (fill_null_weights), or nullptr
    const void *o;               // offset column, or nullptr
    const void *x[POLS_MAX_FEATURES];
    const int64_t *offs;         // DEVICE offsets of the frame's groups
    int64_t n_groups, n_rows;
    const int64_t *seg_offs;     // split form / prediction pass: long groups cut into segments (ensure_segments) or nullptr: one workgroup per group
    const int32_t *seg_map, *seg_first;
    int64_t n_seg;
    const uint8_t *valid;        // optional, drop family only
    int32_t null_policy;
    int32_t k_user, kt;
    int32_t f32;                 // dtype of coef
    int32_t family, max_iter;
    double tol;
    int32_t res_tiles;           // the resident launches serve the groups of up to this many 256-row tiles, the split launches the others (-1: every group)
    int32_t res_from;            // this resident launch: the groups of MORE than res_from and up to res_to tiles
    int32_t res_to;
    int32_t ts;                  // resident launch: column stride of the LDS tile, 256 x (tiles of its longest group) + 1
    double *part;                // items x k13_part_stride(kt)                                     (the segment tables' extra area, or Work::GlmState)
    double *state;               // n_groups x k13_state_stride(kt)                                 (Work::GlmState)
    int32_t *active;             // the split form's groups that still iterate                      (Work::GlmState)
    double *coef64;              // n_groups x kt: the coefficients for the prediction pass         (Work::GlmCoef)
    // outputs, any may be nullptr
    void *coef;
    int32_t *status;
    double *deviance, *se;
    int32_t *n_iter;
    void *pred, *resid, *linpred;   // n_rows, batch dtype (the prediction launch)
};

// dynamic LDS of a resident workgroup whose longest group spans `tiles` 256-row tiles: `cols` staged columns of `elem` bytes
size_t k13_resident_lds(int kt, int cols, size_t elem, int tiles);
// the most 256-row tiles of a group that stay resident in a workgroup's LDS (0: none) with room for per_cu (1 or 2) workgroups on a CU
int k13_resident_tiles(int kt, int cols, size_t elem, int per_cu);
// the whole iteration of the groups of a.res_from < tiles <= a.res_to, one launch
int k13_resident_launch(pols_ctx *ctx, int dtype, const GlmArgs &a);
// one iteration step of the other groups: the segment pass, then the per-group pass (first: the start values instead of coefficients)
int k13_split_launch(pols_ctx *ctx, int dtype, const GlmArgs &a, bool first);
// pred = mu, resid = y - mu, linpred = eta from a.coef64 over every row of the frame
int k13_predict_launch(pols_ctx *ctx, int dtype, const GlmArgs &a);

}  // namespace pols
