// k7r_robust.hpp -- K7r: heteroskedasticity- / autocorrelation-robust standard errors of mode="statistics" (cov_type HC0..HC3, HAC).
#pragma once
#include "k7_stats.hpp"

namespace pols {

constexpr int K7R_MAXLAGS = 255;   // HAC lags the meat kernel's LDS halo is sized for (31 columns, 128-row tiles: 135 KiB)

struct RobustArgs {
    StatsArgs s;          // the K7 arguments of the same call: staged columns, offsets, Gram matrices, segment tables (seg_offs == nullptr: one
                          // segment per group); s.se / s.tv / s.pv receive the robust standard errors, t- and p-values
    int32_t cov_type;     // POLS_COV_HC0 .. POLS_COV_HAC
    int32_t maxlags;      // HAC: L before the per-group min(L, n - 1); 0 otherwise (the halo rows of the meat kernel)
    int32_t tile;         // rows per LDS tile of the meat kernel (k7r_robust_launch picks it)
    double *prep;         // n_groups x (kt^2 + kt + 2): A^-1, A^-1 X'y, trace(A^-1), factorisation ok        (Work::RobustPrep)
    double *part;         // (segments or groups) x (kt^2 + 1): U'W of the segment's rows, "a leverage reached 1" (Work::RobustMeat)
};

__host__ __device__ inline size_t k7r_prep_stride(int kt) { return (size_t)kt * kt + kt + 2; }
__host__ __device__ inline size_t k7r_part_stride(int kt) { return (size_t)kt * kt + 1; }

// prepare / meat / finish on the stream; the r2 / mae / mse of the call come from K7 (k7_stats_launch) unchanged
int k7r_robust_launch(pols_ctx *ctx, int dtype, const RobustArgs &r);

// the prepare launch alone (r.s, r.prep): A^-1, b, trace(A^-1) and ok per group -- what the cluster-robust statistics (K7c) start from
int k7r_prepare_launch(pols_ctx *ctx, int dtype, const RobustArgs &r);

}  // namespace pols
