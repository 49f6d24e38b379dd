// api_internal.hpp -- what the entry translation units share beyond common.hpp.  Who defines what:
//   api.hip         contexts, options, offsets upload (+ scan_offsets), staging, compact_nulls, segments (ensure_segments), k1_launch,
//                   mark_fallback_kernel; the prediction, sharded, layout and Arrow entries
//   api_stats.hip   statistics mode: pols_least_squares_statistics, its robust and cluster twins, pols_least_squares_influence and their
//                   parameter defaults -- the null-policy level, the fit level and its stages.  Nothing of it is declared here (it uses
//                   check_ctx / check_batch / Staged / unstage_outputs / compact_nulls / ls_core / wide_static / ensure_segments from below)
//   api_static.hip  the static least-squares path: resolve_solve_plan, ensure_fallback_epoch, k1_valu_takes, pick_static_route, ls_core,
//                   wide_static, pols_least_squares, pols_multi_target_least_squares, pols_debug_static_route
//   api_dynamic.hip the dynamic entries: the prologue (DynState), the cached per-frame tables, pick_rls_route / pick_rolling_route and one
//                   function per route, pols_recursive_least_squares, pols_rolling_least_squares and their parameter defaults.  Nothing of it
//                   is declared here: no other translation unit calls into it (it uses check_ctx / check_batch / Staged / stage_inputs /
//                   unstage_outputs / aligned16 from below and fail / grow / ensure_scratch / upload_small / upload_offsets from common.hpp)
//   api_fits.hip    the K10-K14, K16 and K17 fit entries
#pragma once

#include <vector>

#include "common.hpp"
#include "dyn_prep.hpp"
#include "k8_wide.hpp"
#include "table_layout.hpp"

namespace pols {

int check_ctx(pols_ctx *ctx);
int check_batch(const pols_batch *b, const pols_out *o, int max_features = POLS_MAX_FEATURES);
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One work buffer for the regions declared on `cv` (scratch_carve.hpp): ONE allocation of their total, then every slot points into it.
// The buffer is a Work member of the context, or one that grow() keeps across calls (a cached table, the K3c granules).
static inline int carve(pols_ctx *ctx, Work w, const Carve &cv) {
    void *base = nullptr;
    const int rc = ensure_scratch(ctx, w, cv.total(), &base);
    if (!rc) cv.place(base);
    return rc;
}
static inline int carve(CachedTable &t, const Carve &cv) {
    void *base = nullptr;
    const int rc = grow(t, cv.total(), &base);
    if (!rc) cv.place(base);
    return rc;
}

// Host-resident batch: stage every column into device scratch (PCIe-inclusive path).
struct Staged {
    const void *y = nullptr, *w = nullptr;
    const uint8_t *valid = nullptr;
    std::vector<const void *> x;     // n_features column pointers (device)
    void *coef = nullptr, *pred = nullptr, *resid = nullptr;
    int32_t *status = nullptr;
};

int stage_inputs(pols_ctx *ctx, const pols_batch *b, int64_t coef_rows, int kt, const pols_out *o, Staged *st);
int unstage_outputs(pols_ctx *ctx, const pols_batch *b, int64_t coef_rows, int kt, const pols_out *o, const Staged &st);
int fill_null_weights(pols_ctx *ctx, const pols_batch *b, Staged *st);

// handle_nulls (src/expressions.rs:255-296) for the entries that work on FILTERED rows: the batch as the policy leaves it --
// device columns compacted inside every group (dyn_prep.hip: count pass, host prefix over the per-group counts, scatter pass),
// new host offsets, nothing null any more (weights included: a null weight is 1e-24, least_squares.py:193).
struct Compacted {
    pols_batch bb;
    std::vector<int64_t> offs;
    std::vector<const void *> xcols, ycols;    // compacted features / targets (ycols[0] == bb.y)
    Staged st;                                  // the ORIGINAL rows on the device (for predictions over every row)
    const int64_t *d_offs = nullptr;            // ... and their offsets
    const uint8_t *vbytes = nullptr;            // row validity (device)
    RowCompactArgs ra;                          // the compaction's tables (slab bases: valid until the next compaction)
};
// `targets` (n_targets >= 1 pointers living where b->mem says) replace b->y as the leading columns: the multi-target mask of
// ex.rs:539-548 is over every target (and, unless drop_y_zero_x, every feature).  n_targets == 0: the single target b->y.
int compact_nulls(pols_ctx *ctx, const pols_batch *b, int policy, Compacted *c, const void *const *targets = nullptr, int n_targets = 0);

// What one pass over the host offsets yields (upload_offsets keeps it in the context, pols_debug_static_route reads it directly).
struct OffsetsScan {
    int64_t max_rows = 0, min_rows = 0;      // min_rows: fewest rows of a NON-EMPTY group (0: no group has rows)
    int64_t tail_group = -1;                 // the last group that has rows: its chunk grid may cross the end of the columns
    int64_t wave_overflow = 0;               // rows beyond the 1 021 (+ 3 of chunk-grid slack) a wave-per-group f32 kernel keeps resident
    int32_t small_mask = 0;                  // which of K6s' team sizes the frame has groups for
    int64_t hist_cnt[48] = {0}, hist_rows[48] = {0};   // groups / rows by size bucket b: 2^(b-1) < rows <= 2^b (bucket 0: 0 or 1 rows)
    bool aligned[2] = {false, false};        // every group start AND size a multiple of 2 / of 4 rows
};
// false: the offsets are not ascending
bool scan_offsets(const int64_t *offs, int64_t n_groups, OffsetsScan *s);

// ------------------------------------------------------------------ static least squares (api_static.hip)
// The reference's dispatcher (src/expressions.rs:366-387) resolved once per call: the branch, its penalties, and the numerical policy of
// the factorisation and of the fix-up pass behind it.
enum class SolveBranch : int { Ols, Ridge, Enet };
struct SolvePlan {
    SolveBranch branch = SolveBranch::Ols;
    double ridge_alpha = 0.0, enet_l1 = 0.5;
    double chol_noise = 0.0;     // a pivot within this (relative) of its diagonal entry is rounding noise around an exact 0
    double pivot_tol = 0.0;      // groups with a pivot d_j <= pivot_tol * (G_jj + alpha) are flagged for the fix-up pass: the measured conditioning
                                 // threshold (10^-1.5 f32 / 1e-6 f64 batches, DESIGN.md "K6 fix_up") on the OLS branch and f32 ridge, else chol_noise
    double rc_factor = -1.0;     // singular-value cut-off of the minimum-norm solver (< 0: eps * max(fit rows, columns) of the group)
    int fix_mode = 0;            // FixMode: the solver the fix-up pass runs on a flagged group
    int lu_fallback = 0;         // engines with an in-kernel LU: a failed Cholesky is retried there (solve_ridge, ls.rs:358-363) -- set for f64 batches only
    bool enet() const { return branch == SolveBranch::Enet; }
    bool ols() const { return branch == SolveBranch::Ols; }
    // (an engine that re-solves a flagged group IN the kernel with LU does so on the same Gram matrix: only a genuinely failed
    // factorisation -- a non-positive or noise pivot -- may take that route.  lu_fallback is set for f64 batches only: under solve_method
    // None / "chol" an f32 batch's ill-conditioned ridge groups get the reference's chain in f64 from the fix-up pass on every route, at
    // pivot_tol.  An explicit "lu" still runs the in-kernel LU of K2 / the streamed solve, which consults no pivot_tol.)
    double in_kernel_pivot_tol() const { return lu_fallback ? chol_noise : pivot_tol; }
};
// POLS_OK, or the POLS_ERR_PANIC of the reference's own argument checks.  n_targets > 1: solve_multi_target (minimum-norm fix-up, rcond honoured).
int resolve_solve_plan(const pols_ols_params *p, int dtype, int kt, int n_targets, SolvePlan *out);
// the device word the solvers stamp when they flag a group (allocated on first use), and this call's epoch
int ensure_fallback_epoch(pols_ctx *ctx);
// shapes the register-resident VALU engine (K1) takes; `aligned`: OffsetsScan::aligned of the dtype
bool k1_valu_takes(const Options &opt, bool aligned, bool f32, int kt, int64_t max_rows, bool has_w = false);

#if defined(__HIPCC__)
// every group is handed to the fix-up pass (api.hip)
__global__ void __launch_bounds__(256) mark_fallback_kernel(const int64_t *offs, int64_t n_groups, int32_t *status, int32_t *fb_flag, int32_t epoch, int only_if_not_empty);
#endif

// What the statistics entry needs back from the solve: the staged columns, the device offsets and (when the streamed
// path ran) the Gram matrices it already produced.  With `info` the outputs are left on the device (no unstage).
struct LsInfo {
    Staged st;
    const int64_t *d_offs = nullptr;
    double *gram = nullptr;
};
int ls_core(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, pols_out *o, LsInfo *info);
// 32 .. 1024 columns (K8).  With `info` (the statistics entry) the outputs stay on the device and the kernel arguments are handed back.
struct WideInfo {
    Staged st;
    WideArgs a;
};
int wide_static(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, pols_out *o, int kt, const SolvePlan &plan,
                const void *const *y_cols = nullptr, int m = 1, void *const *pred_cols = nullptr, WideInfo *info = nullptr);

}  // namespace pols

// Long groups cut into segments (the streamed static path, the statistics of long groups): a group is one workgroup in those
// kernels, so ONE regression over a 10M-row frame used to be one CU's work.  Groups longer than two segments are cut into pieces
// of about N / (8 x CUs) rows (256-row multiples), the others are one segment each; tables in ctx->seg_cache -- segment offsets,
// segment -> group, group -> first segment -- followed by `extra_per_seg` bytes per segment for the caller's partial results.
// n_seg = 0: nothing is longer than two segments (or POLS_NO_SPLIT).  Cached per frame.  (SegTables and its layout: table_layout.hpp)
// ids (size classes): the tables cover only the listed groups (ascending), `offs` holds (start, end) PAIRS per segment, `map` gives the segment's
// position in the list and `first` is indexed by list position; class_key tells such tables apart in the cache (0 = the whole frame).
int ensure_segments(pols_ctx *ctx, const pols_batch *b, int64_t max_rows, size_t extra_per_seg, SegTables *t,
                    const std::vector<int32_t> *ids = nullptr, int64_t class_key = 0);
