/*
 * pols_mi355x.h -- C-ABI of libpols_mi355x.so, the MI355X (gfx950) batched
 * least-squares engine that replaces the solve path of azmyrajab/polars_ols.
 *
 * The boundary sits at the seam between the reference's plugin layer
 * (src/expressions.rs) and its solver layer (src/least_squares.rs), i.e. at the
 * `use crate::least_squares::{...}` import of src/expressions.rs:15-18.  Each
 * entry point below names the reference functions it replaces; INTEGRATION.md
 * shows the `extern "C"` block a maintainer of the reference would add to
 * src/expressions.rs to bind them.
 *
 * Conventions
 *  - plain C: pointers + sizes, no C++/torch types, no exceptions or panics cross
 *    the boundary.  Every entry returns POLS_OK (0) or a negative pols_error;
 *    pols_last_error() returns a thread-local message for the last failure.
 *    The reference's `panic!/assert!` cases (src/least_squares.rs:231,335,349,
 *    366,404-413) map to POLS_ERR_PANIC with the reference's message.
 *  - the caller owns every input / output buffer; the library owns only device
 *    scratch and the HIP stream inside a pols_ctx.  A pols_ctx may be used by
 *    one thread at a time; create one per thread (Polars calls plugins from a
 *    rayon pool, README.md:19).
 *  - data layout: struct-of-arrays, exactly what Polars hands a plugin -- one
 *    contiguous buffer per column (src/expressions.rs:22-63 is the copy into a
 *    row-major matrix that this library deletes).  Rows of one group are
 *    contiguous: group g owns rows [group_offsets[g], group_offsets[g+1]).
 *    A single un-grouped call (what the reference plugin receives per group) is
 *    n_groups = 1, group_offsets = {0, n}.
 *  - `mem` says where ALL data pointers of a batch / out live (HOST: the library
 *    stages through its own device scratch, PCIe-inclusive; DEVICE: zero-copy,
 *    asynchronous on the context's stream).  group_offsets and x_cols (the array
 *    of column pointers itself) are always HOST arrays.
 *  - NaN marks undefined rows of rolling outputs, like src/least_squares.rs:864.
 *  - there is NO CPU fallback: if no gfx950 device is usable every compute entry
 *    fails with POLS_ERR_NO_DEVICE.
 */
#ifndef POLS_MI355X_H
#define POLS_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POLS_MAX_FEATURES 32        /* size of the fixed kernel-argument column arrays; wider calls use device pointer tables */
#define POLS_MAX_FEATURES_STATISTICS 1024 /* pols_least_squares_statistics: features incl. the intercept column */
#define POLS_MAX_FEATURES_DYNAMIC 1024 /* pols_recursive_least_squares / pols_rolling_least_squares (the reference's README
                                          benchmark runs them at 100 features; beyond 128 the k x k state of a chunk lives in
                                          HBM: correct, but every row costs O(k^2) L2 traffic) */
#define POLS_MAX_FEATURES_STATIC 1024 /* pols_least_squares / pols_predict: the reference's own wide cases (tests/benchmark.py
                                         at 100 features, test_elastic_net and test_fit_wide up to 1 000) */

typedef enum {
    POLS_OK = 0,
    POLS_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, unsorted offsets ...) */
    POLS_ERR_UNSUPPORTED = -2, /* valid request this build has no kernel for (message says which) */
    POLS_ERR_HIP = -3,         /* HIP runtime error (message carries hipGetErrorString) */
    POLS_ERR_PANIC = -4,       /* the reference would panic!/assert! on these arguments */
    POLS_ERR_NO_DEVICE = -5    /* no usable gfx950 device; there is no CPU fallback */
} pols_error;

typedef enum { POLS_F32 = 0, POLS_F64 = 1 } pols_dtype;
typedef enum { POLS_MEM_HOST = 0, POLS_MEM_DEVICE = 1 } pols_mem;

/* SolveMethod, src/least_squares.rs:41-65; POLS_SOLVE_AUTO == Option::None. */
typedef enum {
    POLS_SOLVE_AUTO = 0, POLS_SOLVE_QR = 1, POLS_SOLVE_SVD = 2, POLS_SOLVE_CHOL = 3,
    POLS_SOLVE_LU = 4, POLS_SOLVE_CD = 5, POLS_SOLVE_CD_ACTIVE_SET = 6
} pols_solve_method;

/* NullPolicy, src/least_squares.rs:67-91. */
typedef enum {
    POLS_NULL_IGNORE = 0, POLS_NULL_ZERO = 1, POLS_NULL_DROP = 2, POLS_NULL_DROP_ZERO = 3,
    POLS_NULL_DROP_Y_ZERO_X = 4, POLS_NULL_DROP_WINDOW = 5
} pols_null_policy;

/* Per-group status written to pols_out.status. */
typedef enum {
    POLS_GROUP_OK = 0,
    POLS_GROUP_FALLBACK = 1, /* Cholesky failed, the reference's fallback solver was taken (ls.rs:299-327); also every group with FEWER rows
                              * than columns under solve_method None / "svd": the reference picks the SVD for it by shape (ls.rs:224-231).
                              * "Failed" includes the conditioning rule of the OLS branch and of f32 ridge: a pivot d_j <= pivot_tol (G_jj + alpha)
                              * with pivot_tol = 10^-1.5 for f32 batches and 1e-6 for f64 ones, the measured ratios below which a normal-equation
                              * solve leaves the parity tolerance (1e-4 / 1e-6).  Such a group is re-solved in f64 by the reference's own solver
                              * for the call: its values are the reference's, only the status tells. */
    POLS_GROUP_EMPTY = 2,    /* no rows: coefficients are zeros (src/expressions.rs:357-359) */
    POLS_GROUP_NOT_CONVERGED = 3, /* coordinate descent hit max_iter (result still returned, like the reference) */
    POLS_GROUP_BAD_DOF = 4   /* statistics only: degrees of freedom <= 0; the reference panics the whole query here
                                (src/statistics.rs:131-134), a batched launch marks the group, writes NaN standard
                                errors / t / p for it and carries on -- the host decides whether to raise */
} pols_group_status;

typedef struct pols_ctx pols_ctx;

/* ---- context ------------------------------------------------------------ */
int pols_device_count(void);
const char *pols_version(void);
const char *pols_last_error(void);
/* device_id: HIP ordinal.  Creates a private non-blocking stream. */
int pols_create(int device_id, pols_ctx **out);
void pols_destroy(pols_ctx *ctx);
/* Borrow the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream).  The handle is used as
 * given: NULL is HIP's null (legacy default) stream -- which is what torch's default stream is.
 * pols_use_private_stream() goes back to the context's own stream.  A context's scratch buffers are shared by all of its
 * calls: when the stream CHANGES the new stream is made to wait (one event) for what the old one still has in flight, so
 * calls of one context issued under different streams execute in issue order; use one context per stream for concurrency. */
int pols_set_stream(pols_ctx *ctx, void *hip_stream);
int pols_use_private_stream(pols_ctx *ctx);
int pols_synchronize(pols_ctx *ctx);
/* Tuning / diagnostic knobs (engine choices for A/B measurements, debug stamps).  `key` is the name of the matching POLS_*
 * environment variable, with or without the prefix; value NULL restores the default.  The environment is read ONCE, in
 * pols_create(); no compute entry calls getenv. */
int pols_set_option(pols_ctx *ctx, const char *key, const char *value);

/* ---- problem description ------------------------------------------------- */

/* OLSKwargs (src/expressions.rs:298-308) with the Python defaults of
 * polars_ols/least_squares.py:101-107 (see pols_ols_params_default).  has_* == 0 <=> Option::None. */
typedef struct {
    double alpha;
    double l1_ratio;
    int32_t has_l1_ratio;
    int64_t max_iter;
    double tol;
    int32_t positive;
    int32_t solve_method; /* pols_solve_method */
    double rcond;
    int32_t has_rcond;
    int32_t null_policy;  /* pols_null_policy; "ignore" is the OLS default */
} pols_ols_params;
void pols_ols_params_default(pols_ols_params *p);

/* RLSKwargs (src/expressions.rs:310-316; defaults polars_ols/least_squares.py:137-140). */
typedef struct {
    double half_life;
    int32_t has_half_life;
    double initial_state_covariance;        /* default 10.0 */
    const double *initial_state_mean;       /* HOST, n_features + add_intercept values, or NULL */
    int32_t null_policy;                    /* default "drop" */
} pols_rls_params;
void pols_rls_params_default(pols_rls_params *p);

/* RollingKwargs (src/expressions.rs:318-325; defaults polars_ols/least_squares.py:156-160). */
typedef struct {
    int64_t window_size;
    int64_t min_periods;  /* < 0 <=> None -> min(k, window) (ls.rs:860) */
    int32_t use_woodbury; /* < 0 <=> None -> k > 60 (ls.rs:863).  DIVERGENCE: only the default is reproduced -- up to 32 features the
                             window state is X'X (NonWoodburyState, ls.rs:669-735) whatever this field says; from 33 features the
                             inverse is propagated (WoodburyState, :737-787).  use_woodbury = 1 below 33 features (tested by the reference
                             at tests/test_ols.py:718-772) is accepted and ignored: same mathematics, different rounding */
    double alpha;         /* 0 <=> None */
    int32_t null_policy;  /* dataclass default "drop_window"; the namespace method passes "drop" */
} pols_rolling_params;
void pols_rolling_params_default(pols_rolling_params *p);

/* EXTENTS.  Every pointer below names exactly the extent its comment gives ("n_rows", "n_groups x kt", ...): no entry uses a value in
 * front of a column's first element or behind its last one -- a load that reaches past an end (the 16-byte chunk that crosses it, a
 * neighbouring group's rows in a shared chunk, a tile's halo) is clamped into the column or its lanes are SELECTED away, never
 * multiplied by zero, so what lies next to a column, NaN or not, cannot reach a result -- and no entry writes outside an output's
 * extent.  Every element of a requested output is written by every successful call; where the text below is silent about an element
 * (the rows of an empty or failed group, rows before min_periods, a masked row's prediction) it holds what the reference has there: NaN
 * where the reference has a null / NaN, never what the buffer held before.  A call that returns an error code from its argument
 * checks has written nothing.  Groups are independent: what one group's rows hold (Inf, NaN, huge values) does not change another
 * group's results.
 * ALIGNMENT of DEVICE batches (mem == POLS_MEM_DEVICE; host buffers may sit anywhere).  Every per-row COLUMN, input or output, starts
 * on a 16-byte boundary: y, every x_cols[j], weights, the further input columns of an entry (pols_glm_params.offset,
 * pols_iv_params.z_cols, multi-target y_cols) and the per-row outputs pred, resid, multi-target pred_cols, pols_predict's pred_out,
 * the pols_influence_out row fields, pols_glm_out.linpred and pols_rlm_out.weights; anything else is POLS_ERR_INVALID ("device
 * columns must be 16-byte aligned").  coef, status, valid, the cluster id columns and the per-group outputs (statistics, the fit
 * entries' f64 / int32 / int64 tables) need only the alignment of their element type; the dynamic entries take their row-parallel
 * tile kernels only when coef is 16-byte and valid 4-byte aligned and fall back to the chunk kernels otherwise. */
typedef struct {
    int32_t dtype;                /* pols_dtype of y / x / weights and of every output */
    int32_t mem;                  /* pols_mem of the data pointers below */
    int64_t n_rows;
    int64_t n_groups;
    const int64_t *group_offsets; /* HOST, n_groups + 1 ascending values, [0] == 0, [n_groups] == n_rows */
    int32_t n_features;           /* user features, excluding the intercept */
    const void *y;                /* target column, exactly n_rows values; device: 16-byte aligned */
    const void *const *x_cols;    /* HOST array of n_features column pointers, each exactly n_rows values; device: 16-byte aligned */
    const void *weights;          /* sample_weights column or NULL (polars_ols/least_squares.py:190-196).  A null (NaN) weight acts as
                                     the weight 1e-24 -- sqrt_w = w.sqrt().fill_null(1e-12), least_squares.py:193 -- in every entry:
                                     the fill is a device pass behind this boundary (skipped when null_free is set) */
    const uint8_t *valid;         /* optional row validity, 1 byte per row (1 = valid), n_rows bytes at any address, or NULL = all valid */
    int32_t add_intercept;        /* append a ones column LAST, named "const" (least_squares.py:184-188) */
    uint64_t offsets_generation;  /* 0: group_offsets is content-checked on every call (hash, then memcmp against the copy the
                                     library keeps of what it last uploaded).  Non-zero: the caller PROMISES that the same
                                     (group_offsets pointer, n_groups, offsets_generation) always names the same content and bumps
                                     the value whenever it rewrites the array -- repeated calls on one frame then cost O(1) on
                                     the host instead of a pass over the offsets */
    int32_t null_free;            /* non-zero: the caller KNOWS that no target / feature / weight value is null (= NaN here) -- what a Polars
                                     / Arrow caller reads off null_count == 0 for free.  The null policy then has nothing to do:
                                     the static entry takes its policy-free kernels and the dynamic entries skip their validity
                                     scan (one pass over the columns + one stream synchronisation per call).  0 = unknown */
} pols_batch;

typedef struct {
    void *coef;      /* static models: n_groups x kt; dynamic (rls / rolling): n_rows x kt; kt = n_features + add_intercept */
    void *pred;      /* n_rows, or NULL; device: 16-byte aligned */
    void *resid;     /* n_rows: ORIGINAL target - predictions (least_squares.py:239), or NULL; device: 16-byte aligned */
    int32_t *status; /* n_groups pols_group_status values, or NULL */
} pols_out;          /* exact extents, every element written (see EXTENTS above); coef and status: element alignment is enough */

/* ---- compute entries ------------------------------------------------------ */

/* Replaces, for every group in one launch: _get_least_squares_coefficients
 * (src/expressions.rs:351-388) -> solve_ols / solve_ridge / solve_elastic_net
 * (src/least_squares.rs:211-240, 342-371, 386-492) and make_predictions
 * (src/expressions.rs:175-195), including the sqrt(w) pre-scaling, the intercept
 * column and the 1/sqrt(w) un-scaling that polars_ols/least_squares.py:163-239
 * performs around the plugin call. */
int pols_least_squares(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, pols_out *o);

/* Replaces solve_recursive_least_squares (src/least_squares.rs:568-598) + the
 * dynamic make_predictions (src/expressions.rs:184,640-645); one sequence per group.
 * RAW columns go in (both dynamic entries): b->weights, b->add_intercept and the null policy are honoured on the device --
 * sqrt(w) scaling of target and features with a null weight acting as 1e-24 (polars_ols/least_squares.py:190-196), the ones
 * column appended LAST, compute_is_valid_mask for p->null_policy from the NaNs (= nulls) of the scaled columns
 * (src/expressions.rs:201-228; skipped when b->valid is given or b->null_free is set), nulls -> 0 (ex.rs:603, 629, 656, 683),
 * predictions masked by the validity (ex.rs:640-645, 695-700) and un-scaled by 1 / sqrt(w) (ls.py:234-235).  coef has
 * kt = n_features + add_intercept columns; p->initial_state_mean has kt values.
 * A column that is exactly zero for a stretch keeps its decayed information, as in the exact recursion, on every route: the
 * row-parallel forms that truncate a finite half-life's memory extend a tile's carry-in past the stretch ("Silent
 * columns").  Not handled: near-silent columns (a scale drop by more than ~1e3 within the halo) and collinear stretches (no f64
 * method matches those).  After a stretch ends, the P-form routes (> 9 features, POLS_RLS_ENGINE=seq) and the reference itself lose
 * digits for ~25 half-lives of rows (P / ff - k k' r cancels terms of size ff^-stretch). */
int pols_recursive_least_squares(pols_ctx *ctx, const pols_batch *b, const pols_rls_params *p, pols_out *o);

/* Replaces solve_rolling_ols (src/least_squares.rs:848-1032) + dynamic make_predictions.
 * A window whose sums have no Cholesky factorisation is solved by LU with partial pivoting like the reference (ls.rs:732-734) on the
 * default routes: up to 10 features (the row-parallel tile kernel: null-free frames, the drop family with nulls through a source map,
 * "drop_window" with nulls by masking; tests/test_k4_gpu.py::test_rolling_divergence_band_is_pinned) and, since round 6, 11 to 32 features on
 * null-free frames and under the drop family (the wave-per-chunk kernel lists the rows whose sums it could not invert, a follow-up launch runs
 * the LU on them; ::test_rolling_wide_windows_without_an_inverse_take_the_lu): same kind of answer on the same rows.
 * DIVERGENCE (what is left): "drop_window" on a frame WITH nulls at 11 to 32 features -- there such a window yields NaN coefficients where the
 * reference's LU returns whatever a zero or noise pivot produces (inf / NaN / 1e15-sized numbers);
 * pols_set_option("ROLLING_ENGINE", "chunk") selects the kernels that run the LU at those widths.
 * p->use_woodbury is accepted and does not select a code path: up to 8 features (and wherever the chunk kernels run) the sums are
 * re-factored per row, from 9 features on the inverse is propagated with Sherman-Morrison updates whatever the flag says (the
 * reference's WoodburyState arithmetic, ls.rs:737-787, rebuilt from the sums every 128 rows) -- same mathematics, different rounding. */
int pols_rolling_least_squares(pols_ctx *ctx, const pols_batch *b, const pols_rolling_params *p, pols_out *o);

/* Replaces the `predict` plugin body (src/expressions.rs:706-741): row-wise sum_j x[t,j] * coef[t,j].  `coef` holds one
 * coefficient row per input row (coef_rows == n_rows, batch dtype, where `b->mem` says) -- what Polars broadcasts the
 * coefficient struct to before the plugin sees it; b->add_intercept appends the literal 1.0 feature of
 * polars_ols/least_squares.py:479-483; nulls are the caller's (the Python layer zero-fills or masks, :455-491). */
int pols_predict(pols_ctx *ctx, const pols_batch *b, const void *coef, int64_t coef_rows, void *pred_out);
/* The same with the plugin's `null_policy` kwarg (PredictKwargs, ex.rs:708): nulls are NaNs here; features are zero-filled unless the
 * policy is "ignore" (construct_features_array(.., null_policy != Ignore), :725); under "drop" the rows with a null anywhere come
 * back null (:732-738) -- with NaN as the null that is what the un-filled product already is, so POLS_NULL_DROP computes like
 * POLS_NULL_IGNORE.  pols_predict == pols_predict_policy(.., POLS_NULL_IGNORE, ..). */
int pols_predict_policy(pols_ctx *ctx, const pols_batch *b, const void *coef, int64_t coef_rows, int32_t null_policy, void *pred_out);

/* mode="statistics": replaces the plugin `least_squares_statistics` (src/expressions.rs:468-509) and
 * src/statistics.rs:15-156 for every group of the batch.  Per group, on the sqrt(w)-scaled rows the reference's
 * Python layer hands the plugin (polars_ols/least_squares.py:190-196):
 *   coefficients          from the same dispatcher as pols_least_squares (written to out->coef, batch dtype),
 *   r2, mae, mse          compute_residual_metrics (st.rs:15-37) of those coefficients,
 *   std_err, t, p         compute_feature_metrics (st.rs:79-156): (X'X + alpha I)^-1 by Cholesky (failure -> NaN),
 *                         its own coefficients inv . X'y, RSS / df with df = n - p (alpha == 0) or n - trace(inv),
 *                         two-sided Student-t p-values.
 * The six statistic arrays are always f64 (the reference's struct fields are Float64) and live where `b->mem` says;
 * any of them may be NULL.  out->pred / out->resid are honoured as in pols_least_squares; out->status receives
 * POLS_GROUP_BAD_DOF where the reference would have hit its df > 0 assertion. */
/* Several targets regressed on the same features: replaces the plugin `multi_target_least_squares`
 * (src/expressions.rs:521-591) and solve_multi_target (src/least_squares.rs:243-260).  `b->y` is ignored; `y_cols` holds
 * n_targets column pointers (the fields of the reference's target struct), `pred_cols` n_targets output columns (or NULL),
 * `coef` n_groups x n_targets x (n_features + intercept) in the batch dtype (or NULL), `status` n_groups (or NULL); all
 * live where `b->mem` says.  Unconstrained OLS / ridge with solve_method None or "svd" only, like the reference's Python
 * checks (polars_ols/least_squares.py:303-318, reported as POLS_ERR_PANIC).  Null policies as in the plugin body: the joint
 * validity mask over every target and (unless drop_y_zero_x) every feature (ex.rs:539-548), the fit on the rows it leaves, then
 * predictions for EVERY row from the zero-filled features, masked to NaN under "drop" (ex.rs:566-585). */
int pols_multi_target_least_squares(pols_ctx *ctx, const pols_batch *b, const void *const *y_cols, int32_t n_targets,
                                    const pols_ols_params *p, void *const *pred_cols, void *coef, int32_t *status);

typedef struct pols_stats_out {
    double *r2, *mae, *mse;                 /* n_groups                         */
    double *std_err, *t_values, *p_values;  /* n_groups x (n_features + intercept), row-major */
} pols_stats_out;

int pols_least_squares_statistics(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, pols_out *out,
                                  const pols_stats_out *stats);

/* Robust standard errors for mode="statistics" (extends pols_least_squares_statistics above; the reference's
 * compute_feature_metrics, src/statistics.rs:79-156, has only the constant-variance form).  Per group, on the same rows,
 * sqrt(w) scaling and ones column as pols_least_squares_statistics, with A = X'X + alpha I, b = A^-1 X'y its side-car
 * coefficients, e_i = y_i - x_i'b and the leverage h_i = x_i' A^-1 x_i:
 *   u_i = c_i e_i x_i,  c_i = 1 (HC0, HC1, HAC), (1 - h_i)^-1/2 (HC2), (1 - h_i)^-1 (HC3),
 *   S   = sum_i u_i u_i', plus for HAC sum_{l=1..L} (1 - l / (L + 1)) sum_i (u_i u_{i-l}' + u_{i-l} u_i') with
 *         L = min(maxlags, n - 1), lags over the group's rows in their order (no small-sample factor: HAC, maxlags 0 == HC0),
 *   V   = A^-1 S A^-1 (times n / df for HC1),  std_err_j = sqrt(V_jj),  t_j = b_j / std_err_j,  p_j as the non-robust entry.
 * df, r2 / mae / mse, the coefficients, status and the failure rules are those of pols_least_squares_statistics; HC2 / HC3
 * also give NaN standard errors / t / p to a group with a row of 1 - h_i < 1e-10.  POLS_COV_NONROBUST calls
 * pols_least_squares_statistics.  Up to 31 columns (incl. the intercept) and maxlags 0..255; wider calls and longer lags
 * return POLS_ERR_UNSUPPORTED, a negative maxlags (HAC) or an unknown cov_type POLS_ERR_INVALID. */
enum {
    POLS_COV_NONROBUST = 0,
    POLS_COV_HC0 = 1,
    POLS_COV_HC1 = 2,
    POLS_COV_HC2 = 3,
    POLS_COV_HC3 = 4,
    POLS_COV_HAC = 5,         /* Newey-West: Bartlett weights over maxlags lags */
    POLS_COV_CLUSTER = 6,     /* one-way cluster-robust: pols_least_squares_statistics_cluster only */
    POLS_COV_CLUSTER2 = 7     /* two-way cluster-robust: pols_least_squares_statistics_cluster only */
};

typedef struct pols_cov_params {
    int32_t cov_type;         /* POLS_COV_* */
    int32_t maxlags;          /* HAC only */
} pols_cov_params;

/* cov_type = POLS_COV_NONROBUST, maxlags = 0 */
void pols_cov_params_default(pols_cov_params *c);

int pols_least_squares_statistics_robust(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_cov_params *cov,
                                         pols_out *out, const pols_stats_out *stats);

/* Cluster-robust standard errors for mode="statistics" (no reference counterpart; statsmodels' cov_type="cluster", Stata's
 * vce(cluster ...)).  Per group, on exactly the rows, sqrt(w) scaling, ones column, A = X'X + alpha I, b and df of
 * pols_least_squares_statistics_robust, with e_i = y_i - x_i'b and u_i = e_i x_i:
 *   one-way  the clusters are the distinct ids among the group's kept rows, G their number;  s_c = sum_{i in c} u_i,
 *            z_c = A^-1 s_c,  V_jj = q sum_c z_cj^2  with q = G / (G - 1) (N - 1) / df when use_correction (Stata's CR1),
 *            1 otherwise (N: the group's kept rows);
 *   two-way  ids A and B, AB = the distinct (a, b) pairs:  V_jj = q_A sum z_A^2 + q_B sum z_B^2 - q_AB sum z_AB^2, each q with
 *            its own G (Cameron-Gelbach-Miller);
 *   se_j = sqrt(V_jj), t_j = b_j / se_j, p_j two-sided Student-t with G - 1 degrees of freedom (two-way: min(G_A, G_B) - 1) --
 *   the Stata / statsmodels convention, deliberately not K7's df.
 * NaN se / t / p for a group with G < 2 (two-way: min(G_A, G_B) < 2), with df <= 0 under the correction, or whose factorisation
 * failed; two-way, a coefficient with V_jj < 0 alone.  r2 / mae / mse, the coefficients and status are those of
 * pols_least_squares_statistics, bit for bit.  Sums run in a fixed order (clusters by ascending id, rows in frame order inside a
 * cluster), so results are bit-identical from run to run.  ids[w] hold one int64 per row in the batch's row order, where b->mem says;
 * they follow their rows through the null policy (a cluster whose rows all dropped does not count).  n_clusters (optional, where
 * b->mem says): n_groups x 1 (G) or n_groups x 2 (G_A, G_B) int64.  Up to 31 columns (incl. the intercept) and fewer than 2^31 rows;
 * larger calls return POLS_ERR_UNSUPPORTED; a NULL id column or a cov_type other than CLUSTER / CLUSTER2 POLS_ERR_INVALID.  The robust entry above
 * rejects POLS_COV_CLUSTER / CLUSTER2 with POLS_ERR_INVALID. */
typedef struct pols_cluster_params {
    int32_t cov_type;         /* POLS_COV_CLUSTER (ids[0]) or POLS_COV_CLUSTER2 (ids[0], ids[1]) */
    int32_t use_correction;   /* 1: G / (G - 1) (N - 1) / df per way (default); 0: none */
    const int64_t *ids[2];    /* cluster id per row */
    int64_t *n_clusters;      /* optional output */
} pols_cluster_params;

/* cov_type = POLS_COV_CLUSTER, use_correction = 1, ids = n_clusters = NULL */
void pols_cluster_params_default(pols_cluster_params *c);

int pols_least_squares_statistics_cluster(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_cluster_params *cl,
                                          pols_out *out, const pols_stats_out *stats);

/* Per-row influence diagnostics and prediction intervals (no reference counterpart; statsmodels' OLSInfluence and
 * get_prediction().summary_frame()).  Per group g, on the rows F_g that pols_least_squares_statistics_robust fits -- the same null-policy
 * filtering / zero-filling, sqrt(w) scaling (a null weight acting as 1e-24) and ones column last -- with x~_i = sqrt(w_i) x_i,
 * y~_i = sqrt(w_i) y_i, p = n_features + intercept, A = X~'X~ + alpha I over F_g, b = A^-1 X~'y~ (the side-car coefficients of the
 * statistics entries), n = |F_g| and their df (n - p, or n - trace A^-1 when alpha > 0):
 *   sigma2 (group)     sum_{i in F_g} e~_i^2 / df  with  e~_i = y~_i - x~_i'b
 *   df, t_crit (group) df as above; t_crit = the (1 - (1 - level) / 2) quantile of Student-t with df degrees of freedom
 *   leverage           h_i = x~_i' A^-1 x~_i
 *   student_internal   r_i = e~_i / sqrt(sigma2 (1 - h_i))
 *   student_external   t_i = r_i sqrt((df - 1) / (df - r_i^2)); NaN when df - 1 <= 0 or df - r_i^2 <= 0
 *   cooks_d            r_i^2 h_i / (p (1 - h_i))
 *   dffits             t_i sqrt(h_i / (1 - h_i))
 *   se_mean            sqrt(sigma2 h_i / w_i): the standard error of x_i'b in the target's units
 *   se_obs             sqrt(sigma2 (1 + h_i) / w_i): statsmodels' WLS convention, var_resid = scale / weights
 *   mean_lo / mean_hi  x_i'b -+ t_crit se_mean          obs_lo / obs_hi   x_i'b -+ t_crit se_obs      (x_i'b un-scaled)
 * High leverage: a fitted row with 1 - h_i < 1e-10 has NaN in student_internal, student_external, cooks_d and dffits; its leverage,
 * standard errors and intervals are written, the rest of its group is unaffected.
 * Rows outside the fit (the forecasting idiom: a null target under a drop-family policy): a row of the group that the policy left out
 * of F_g is scored as a NEW OBSERVATION when every feature is non-null after the policy's own fill and its weight is non-null --
 * leverage (the same quadratic form, not bounded by 1), se_mean, se_obs and the four interval ends; its four influence measures are
 * NaN.  With a null feature or weight left it is NaN everywhere.  Under "ignore" nothing is masked: NaNs propagate arithmetically.
 * Penalised / constrained fits: like the statistics entries everything rests on the side-car b whatever the dispatcher solved;
 * l1_ratio / positive / solve_method affect only out->coef / pred / resid.
 * A group whose factorisation failed or whose df <= 0 has NaN in every per-row output and in sigma2 / t_crit; out->status is what
 * pols_least_squares_statistics writes (POLS_GROUP_BAD_DOF included), as are out->coef / pred / resid, bit for bit.
 * f32 batches: the side-car b takes one step of iterative refinement in f64 first (the Gram matrix of an f32 frame is summed in f32
 * pieces; a row's residual is a difference that keeps no digits of such a b where it nearly vanishes); f64 batches use it as it is.
 * Everything is computed in f64; per-row arrays are stored in the batch dtype, per-group arrays as f64; all live where b->mem says and
 * any may be NULL.  Sums run in a fixed order without atomics: two runs are bit-identical.  Parameter validation as the robust entry
 * (null policy range, a validity mask only under a drop-family policy, up to 31 columns incl. the intercept, else
 * POLS_ERR_UNSUPPORTED); a level outside (0, 1) is POLS_ERR_INVALID. */
typedef struct pols_influence_params {
    double level;             /* 0 < level < 1, default 0.95 */
} pols_influence_params;

/* level = 0.95 */
void pols_influence_params_default(pols_influence_params *q);

typedef struct pols_influence_out {
    void *leverage, *student_internal, *student_external, *cooks_d, *dffits,
         *se_mean, *se_obs, *mean_lo, *mean_hi, *obs_lo, *obs_hi;   /* n_rows, batch dtype */
    double *sigma2, *df, *t_crit;                                   /* n_groups, f64 */
} pols_influence_out;

int pols_least_squares_influence(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_influence_params *q,
                                 pols_out *out, const pols_influence_out *infl);

/* the per-row fields of pols_influence_out, in its order: bit i of a field mask names the i-th pointer */
enum {
    POLS_INFL_LEVERAGE = 1 << 0, POLS_INFL_STUDENT_INTERNAL = 1 << 1, POLS_INFL_STUDENT_EXTERNAL = 1 << 2, POLS_INFL_COOKS_D = 1 << 3,
    POLS_INFL_DFFITS = 1 << 4, POLS_INFL_SE_MEAN = 1 << 5, POLS_INFL_SE_OBS = 1 << 6, POLS_INFL_MEAN_LO = 1 << 7,
    POLS_INFL_MEAN_HI = 1 << 8, POLS_INFL_OBS_LO = 1 << 9, POLS_INFL_OBS_HI = 1 << 10, POLS_INFL_ALL = (1 << 11) - 1
};

/* Ridge regularisation path with leave-one-out selection of alpha, per group (no reference counterpart; the job of scikit-learn's
 * RidgeCV).  Per group g, the rows F_g are those pols_least_squares fits -- the same null-policy filtering / zero-filling and validity
 * mask rules, sqrt(w) scaling with a null weight acting as 1e-24, the ones column last and PENALISED like any other (the reference
 * adds alpha I to every column, src/least_squares.rs:342-364) -- with x~_i = sqrt(w_i) x_i, y~_i = sqrt(w_i) y_i, n = |F_g|,
 * kt = n_features + intercept.  For every candidate a_j = params.alphas[j]:
 *   A_j = X~'X~ + a_j I,   b_j = A_j^-1 X~'y~,   h_ij = x~_i' A_j^-1 x~_i,
 *   cv_scores[g][j] = (1 / n) sum_{i in F_g} ((y~_i - x~_i'b_j) / (1 - h_ij))^2
 * which is the exact leave-one-out mean squared error of that ridge on the scaled rows (the leverage identity holds because the
 * penalty covers every column: no refit).  Unweighted and without an intercept it is scikit-learn's
 * RidgeCV(fit_intercept=False).cv_results_.mean(0); with sample weights scikit-learn weights the squared errors differently and does
 * not match -- this definition is the project's own.
 * A candidate is UNUSABLE for a group -- its score and its coef_path row are NaN -- when
 *   - A_j has no Cholesky factorisation.  The rule applied, on the computed spectrum s of X~'X~ (Jacobi rotations in f64):
 *     min(s) + a_j <= 16 kt eps (max(s) + a_j), the noise floor the f64 Cholesky of the static entries puts on a pivot; or
 *   - some fitted row has 1 - h_ij < 1e-10 (the HC2 / HC3 rule of the robust statistics), or the score is not a number.
 *   An exact in-sample fit with alpha = 0 is therefore unusable, never "score 0".
 * The chosen candidate is the usable one with the smallest score, the lowest index on an exact tie.  out->coef / pred / resid are
 * those of the chosen candidate, with the shape and null-policy masking of pols_least_squares(alpha = chosen) on that group
 * (predictions un-scaled by 1 / sqrt(w), every row predicted or masked as that entry does).  out->status per group: POLS_GROUP_OK;
 * POLS_GROUP_EMPTY for n = 0 (coefficients zeros, scores / alpha / score NaN, index -1); POLS_GROUP_FALLBACK when NO candidate is
 * usable (index -1; alpha, score, coef, pred, resid NaN).  Groups with n <= kt are legal whenever alpha > 0.
 * The Gram matrix, the decomposition and all scoring run in f64 on the inputs' values, for f32 batches too; coef / coef_path / pred /
 * resid are stored in the batch dtype.  Sums run in a fixed order without atomics: two runs are bit-identical.
 * From pols_ols_params only null_policy is consulted; positive, or has_l1_ratio with l1_ratio > 0, is POLS_ERR_INVALID (no hat
 * matrix).  POLS_ERR_INVALID: alphas == NULL, n_alphas < 1, a negative or non-finite candidate, an unknown null policy, a mask
 * without a drop-family policy.  POLS_ERR_UNSUPPORTED: more than 31 columns incl. the intercept, more than 64 candidates. */
typedef struct pols_ridge_cv_params {
    const double *alphas;     /* HOST array, any order, each >= 0 and finite */
    int32_t n_alphas;
} pols_ridge_cv_params;

/* alphas = NULL, n_alphas = 0 */
void pols_ridge_cv_params_default(pols_ridge_cv_params *q);

typedef struct pols_ridge_cv_out {
    double  *alpha;           /* n_groups: the chosen alpha                              */
    int32_t *alpha_index;     /* n_groups: its index in params.alphas, -1 if none usable */
    double  *score;           /* n_groups: its leave-one-out mean squared error          */
    double  *cv_scores;       /* n_groups x n_alphas, row-major                          */
    void    *coef_path;       /* n_groups x n_alphas x kt, batch dtype                   */
} pols_ridge_cv_out;          /* all live where b->mem says; any may be NULL */

int pols_ridge_cv(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_ridge_cv_params *q, pols_out *out,
                  const pols_ridge_cv_out *cv);

/* Huber / Tukey-bisquare M-estimator per group by iteratively reweighted least squares (no reference counterpart; statsmodels'
 * RLM with its MAD scale).  Per group g, the fitted rows F_g are exactly those pols_least_squares fits -- the same null-policy
 * filtering / zero-filling and validity-mask rules, a null weight acting as 1e-24, the ones column last -- with
 * x~_i = sqrt(w_i) x_i, y~_i = sqrt(w_i) y_i, n = |F_g|, kt = n_features + intercept.  All arithmetic is f64 on the inputs' values,
 * for f32 batches too.
 *   1. Start.  b^0 is the OLS solution on F_g: an f64 Gram matrix and a Cholesky factorisation with the pivot floor of the static
 *      entries' f64 Cholesky -- a pivot fails when d^2 <= 16 kt eps A_jj.
 *   2. Scale.  With r_i = y~_i - x~_i'b^t over F_g:  s = median(|r_i|) / 0.6744897501960817, the normalised MAD about zero.  The
 *      median is exact; for even n it is the mean of the two middle order statistics.
 *   3. Robust weights.  omega_i = psi(u_i) / u_i with u_i = |r_i| / s:
 *        POLS_RLM_HUBER    = 0:  1 for u <= c, else c / u              (default c 1.345)
 *        POLS_RLM_BISQUARE = 1:  (1 - (u / c)^2)^2 for u < c, else 0   (default c 4.685)
 *   4. Update.  b^(t+1) solves (sum omega_i x~_i x~_i') b = sum omega_i x~_i y~_i by the same Cholesky rule.
 *   5. Stop.  Converged when max_j |b^(t+1)_j - b^t_j| <= tol max(max_j |b^(t+1)_j|, 1e-300); otherwise the iteration stops after
 *      max_iter updates with status POLS_GROUP_NOT_CONVERGED and the result is still returned.  n_iter is the number of updates made.
 * Edge rules.
 *   - n = 0: POLS_GROUP_EMPTY, zero coefficients, scale NaN, n_iter 0.
 *   - POLS_GROUP_FALLBACK with NaN coef, pred, resid, scale and weights: n <= kt; a start that is not finite (NaNs under "ignore");
 *     a Cholesky failure at the start or in any update (bisquare can zero out too many rows), or an update that is not finite.
 *   - Scale collapse: s <= 16 eps max_{F_g} |y~_i|, or s not finite.  The iteration stops there AS CONVERGED with the current
 *     coefficients -- an exact fit is not an error.
 *   - The reported scale is the last s computed.  The reported weights are the omega used in the last update that was made: all
 *     ones if none was made, NaN for the rows outside F_g.
 * out->coef / pred / resid have the shape and the null-policy masking of pols_least_squares with those coefficients (predictions
 * un-scaled, resid = y - pred, every row predicted or masked as that entry does); out->status per group as above, else
 * POLS_GROUP_OK.  Sums run in a fixed order without floating-point atomics: two runs are bit-identical.
 * From pols_ols_params only null_policy is read.  POLS_ERR_INVALID: alpha != 0, positive, or has_l1_ratio with l1_ratio > 0; an
 * unknown norm; a non-finite c; max_iter < 1; tol not positive and finite; an unknown null policy; a validity mask without a
 * drop-family policy.  POLS_ERR_UNSUPPORTED: more than 31 columns incl. the intercept; a group too long for a workgroup's LDS
 * with more than 2^22 rows (such groups are walked by ONE workgroup per iteration pass; a form that splits them is not built).
 * There is no Arrow twin of this entry. */
enum { POLS_RLM_HUBER = 0, POLS_RLM_BISQUARE = 1 };

typedef struct pols_rlm_params {
    int32_t norm;             /* POLS_RLM_HUBER / POLS_RLM_BISQUARE          */
    double  c;                /* tuning constant; <= 0: the norm's default   */
    int32_t max_iter;         /* >= 1                                        */
    double  tol;              /* positive and finite                         */
} pols_rlm_params;

/* norm = POLS_RLM_HUBER, c = 0 (the norm's default), max_iter = 50, tol = 1e-8 */
void pols_rlm_params_default(pols_rlm_params *q);

typedef struct pols_rlm_out {
    double  *scale;           /* n_groups: the last s computed               */
    int32_t *n_iter;          /* n_groups: updates made                      */
    void    *weights;         /* n_rows, batch dtype: omega of the last update; device: 16-byte aligned */
} pols_rlm_out;               /* all live where b->mem says; any may be NULL */

int pols_rlm(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_rlm_params *q, pols_out *out,
             const pols_rlm_out *r);

/* Logistic / Poisson generalised linear model per group by iteratively reweighted least squares (no reference counterpart; R's
 * glm / statsmodels' GLM with the canonical link, for every group of the frame in one call).
 * Fitted rows and arithmetic.  Per group g, the fitted rows F_g are exactly those pols_least_squares / pols_rlm fit -- the same
 * null-policy filtering / zero-filling and validity-mask rules, the ones column last -- n = |F_g|, kt = n_features + intercept.  All
 * arithmetic is f64 on the inputs' values, for f32 batches too.
 * Prior weights.  b->weights are prior weights w_i (frequency / variance weights): they multiply the working weight and the deviance
 * terms; a null weight acts as 1e-24.  The rows are NOT scaled by sqrt(w).
 * Offset.  q->offset, optional: o_i, n_rows in the batch dtype, living where b->mem says (16-byte aligned on the device); NULL
 * means 0.  A null (NaN) offset makes its row a null row exactly as a null feature does.
 * Families (canonical links only), eps = 2^-52:
 *   POLS_GLM_BINOMIAL = 0:  mu = clip(1 / (1 + exp(-eta)), eps, 1 - eps),  d(mu) = mu (1 - mu),
 *                           u(y, mu) = y log(y / mu) + (1 - y) log((1 - y) / (1 - mu))  with 0 log 0 = 0,
 *                           domain 0 <= y <= 1 (fractions allowed),  start mu^0 = (y + 0.5) / 2
 *   POLS_GLM_POISSON  = 1:  mu = max(exp(eta), eps),  d(mu) = mu,  u(y, mu) = y log(y / mu) - (y - mu),
 *                           domain y >= 0,  start mu^0 = y + 0.1
 * The deviance is D(mu) = 2 sum_{F_g} w_i u(y_i, mu_i).
 * Iteration.
 *   1. Start.  eta^0 = g(mu^0) (logit / log), D^0 = D(mu^0).  There is no b^0.
 *   2. Update t -> t + 1, over F_g:  W_i = w_i d(mu_i),  z_i = eta_i - o_i + (y_i - mu_i) / d(mu_i);  b^(t+1) solves
 *      (sum W_i x_i x_i') b = sum W_i x_i z_i by the static entries' f64 Cholesky rule -- a pivot fails when d^2 <= 16 kt eps A_jj;
 *      then eta_i = x_i'b^(t+1) + o_i, mu as above, and D^(t+1).
 *   3. Stop.  Converged when |D^(t+1) - D^t| <= tol (|D^(t+1)| + 0.1) (R's glm.control rule); otherwise the iteration stops after
 *      max_iter updates with status POLS_GROUP_NOT_CONVERGED and the result is still returned.  n_iter is the number of updates made.
 * Reported values.  coef = the last b; deviance = D at it; se_j = sqrt([(sum W x x')^-1]_jj) of the matrix factorised in the last
 * update (dispersion 1, what statsmodels reports); out->pred = mu on the response scale, offset included; out->resid = y - mu;
 * linpred = eta per row.  Every row is predicted or masked as pols_least_squares does for the policy (features and offsets
 * zero-filled under every policy but "ignore", "drop" masks the rows outside the fit with NaN -- linpred too).
 * Edge rules.
 *   - n = 0: POLS_GROUP_EMPTY, zero coefficients, deviance / se NaN, n_iter 0.
 *   - POLS_GROUP_FALLBACK with NaN coef, se, deviance, pred, resid and linpred: n <= kt; a fitted row with y outside the family's
 *     domain, or a non-finite value under "ignore"; a Cholesky failure in any update; an update or a deviance that is not finite
 *     (Poisson overflow).
 *   - Complete separation is NOT detected: such a group ends as the stop rule says (the deviance creeps towards 0 while the
 *     coefficients grow), usually as converged with large coefficients and standard errors.
 *   - Otherwise POLS_GROUP_OK.
 * Determinism.  No floating-point atomics, every sum in a fixed order: two runs are bit-identical, HOST and DEVICE batches agree
 * bit for bit.  Groups short enough for a workgroup's LDS are fitted in one launch; longer ones, of any length, are cut into
 * segments and iterate with two launches per update -- the entry then SYNCHRONISES THE STREAM once per update to read how many
 * groups still iterate.  POLS_GLM_ENGINE=split (pols_set_option) sends every group that way.
 * From pols_ols_params only null_policy is read.  POLS_ERR_INVALID: alpha != 0, positive, or has_l1_ratio with l1_ratio > 0; an
 * unknown family; max_iter < 1; tol not positive and finite; an unknown null policy; a validity mask without a drop-family policy.
 * POLS_ERR_UNSUPPORTED: more than 31 columns incl. the intercept.  There is no row limit, no Arrow twin and no sharded entry. */
enum { POLS_GLM_BINOMIAL = 0, POLS_GLM_POISSON = 1 };

typedef struct pols_glm_params {
    int32_t family;           /* POLS_GLM_BINOMIAL / POLS_GLM_POISSON        */
    int32_t max_iter;         /* >= 1                                        */
    double  tol;              /* positive and finite                         */
    const void *offset;       /* n_rows, batch dtype, or NULL                */
} pols_glm_params;

/* family = POLS_GLM_BINOMIAL, max_iter = 25, tol = 1e-8, offset = NULL */
void pols_glm_params_default(pols_glm_params *q);

typedef struct pols_glm_out {
    double  *deviance;        /* n_groups: D at the returned coefficients    */
    double  *se;              /* n_groups x kt: standard errors, dispersion 1 */
    int32_t *n_iter;          /* n_groups: updates made                      */
    void    *linpred;         /* n_rows, batch dtype: eta                    */
} pols_glm_out;               /* all live where b->mem says; any may be NULL */

int pols_glm(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_glm_params *q, pols_out *out,
             const pols_glm_out *r);

/* Elastic-net / lasso regularisation path with K-fold selection of alpha, per group (no reference counterpart: the reference's
 * lasso / elastic_net take one alpha for the whole frame; this is the job of scikit-learn's LassoCV / ElasticNetCV with
 * fit_intercept=False and cv=KFold(n_folds)).  There is no Arrow twin of this entry.
 * Fitted rows.  Per group g, the fitted rows F_g are exactly those pols_least_squares / pols_ridge_cv fit -- the same null-policy
 * filtering / zero-filling and validity-mask rules, a null weight acting as 1e-24, the ones column last -- with
 * x~_i = sqrt(w_i) x_i, y~_i = sqrt(w_i) y_i, n = |F_g|, kt = n_features + intercept.  All arithmetic is f64 on the inputs' values,
 * for f32 batches too.
 * Folds.  n_folds contiguous folds over the FITTED rows in row order: the fitted row of rank r (0-based among F_g) belongs to the
 * fold scikit-learn's KFold(shuffle=False) gives it -- the first n % n_folds folds hold n / n_folds + 1 rows, the rest n / n_folds.
 * With a drop-family policy the result therefore equals "filter, then fit".  n_f is the size of fold f.
 * Candidates.  Explicit: params.alphas is a HOST array in any order, each finite and >= 0.  Automatic: alphas == NULL,
 * n_alphas >= 2, 0 < eps < 1, l1_ratio > 0; per group alpha_max = max_j |X~'y~|_j / (n l1_ratio) over the full data and
 * a_j = alpha_max eps^(j / (n_alphas - 1)) (scikit-learn's grid for fit_intercept=False), formed on the device and returned in
 * alphas_used.  An alpha_max that is not positive and finite makes the group a POLS_GROUP_FALLBACK.
 * Fits.  With G = X~'X~, c = X~'y~ over the rows of a fit and m the NUMBER OF ROWS OF THAT FIT (n - n_f for the training
 * problem of fold f, n for the full data), candidate a minimises the reference's objective (solve_elastic_net,
 * src/least_squares.rs:386-492, cyclic `cd` only) by its iteration in Gram form: one sweep updates j = 0 .. kt - 1 in order,
 *   w_j <- S(c_j - sum_{i != j} G_ji w_i, a m l1_ratio) / (G_jj + a m (1 - l1_ratio)),   S the soft threshold (max(., 0) of it when
 * `positive`), and the fit stops after the first sweep with ||w_new - w_old||_2 < tol, or after max_iter sweeps.  Candidates are
 * visited in order of descending alpha, equal values in index order; the first starts from zeros, each later one from its
 * predecessor's solution.  This is done independently for each of the n_folds training problems and for the full data.
 * Scores.  cv_scores[g][j] = (1 / n_folds) sum_f max(0, yy_f - 2 b'c_f + b'G_f b) / n_f with b the fold-f fit at candidate j and
 * G_f, c_f, yy_f the Gram matrix of the rows of fold f: the unweighted mean over the folds of the validation mean squared error on
 * the scaled rows.  It is computed from the fold's Gram matrix, not from residuals, so its relative accuracy is about
 * eps yy_f / rss_f.  Chosen: the candidate with the smallest finite score, the lowest index on an exact tie; a NaN score is never
 * chosen.
 * Outputs.  out->coef / pred / resid: the full-data path's coefficients at the chosen index, with the shape and the null-policy
 * masking of pols_least_squares with those coefficients.  Because of the warm starts they differ from a cold-started
 * elastic_net(alpha = chosen) by at most the stopping tolerance.  n_iter[g][j] is the largest sweep count among the n_folds + 1
 * fits of candidate j.  coef_path is the full-data path.
 * out->status per group: POLS_GROUP_EMPTY for n = 0 (zero coefficients, NaN scores, index -1); POLS_GROUP_FALLBACK for
 * 0 < n < n_folds, a bad automatic grid or no finite score (coef, pred, resid, alpha, score NaN, index -1); in both cases, and
 * whenever n < n_folds or the automatic grid is bad, cv_scores and coef_path are NaN, n_iter 0, and alphas_used is NaN in automatic
 * mode (the explicit candidates otherwise).  POLS_GROUP_NOT_CONVERGED when the stop rule never fired within max_iter sweeps in one
 * of the chosen candidate's n_folds + 1 fits (results are still returned); POLS_GROUP_OK otherwise.
 * Sums run in a fixed order without floating-point atomics: two runs are bit-identical.
 * From pols_ols_params only null_policy is read.  POLS_ERR_INVALID: l1_ratio outside [0, 1] or not finite; a negative or non-finite
 * candidate; n_alphas < 1, or < 2 in automatic mode; eps outside (0, 1) or l1_ratio == 0 in automatic mode; n_folds outside
 * 2 .. 16; max_iter < 1; tol not positive and finite; an unknown null policy; a validity mask without a drop-family policy.
 * POLS_ERR_UNSUPPORTED: more than 31 columns incl. the intercept; more than 128 candidates. */
typedef struct pols_enet_cv_params {
    const double *alphas;     /* HOST array, any order, each >= 0 and finite; NULL: the automatic grid */
    int32_t n_alphas;
    double  eps;              /* automatic grid: alpha_min / alpha_max, in (0, 1)  */
    double  l1_ratio;         /* in [0, 1]; 1 = lasso                              */
    int32_t n_folds;          /* 2 .. 16                                           */
    int32_t max_iter;         /* >= 1                                              */
    double  tol;              /* positive and finite                               */
    int32_t positive;         /* non-zero: coefficients >= 0                       */
} pols_enet_cv_params;

/* alphas = NULL, n_alphas = 100, eps = 1e-3, l1_ratio = 0.5, n_folds = 5, max_iter = 1000, tol = 1e-5, positive = 0 */
void pols_enet_cv_params_default(pols_enet_cv_params *q);

typedef struct pols_enet_cv_out {
    double  *alpha;           /* n_groups: the chosen alpha                                  */
    int32_t *alpha_index;     /* n_groups: its index among the candidates, -1 if none        */
    double  *score;           /* n_groups: its mean validation error                         */
    double  *cv_scores;       /* n_groups x n_alphas, row-major                              */
    double  *alphas_used;     /* n_groups x n_alphas: every group's candidates               */
    void    *coef_path;       /* n_groups x n_alphas x kt, batch dtype: the full-data path   */
    int32_t *n_iter;          /* n_groups x n_alphas: most sweeps among the n_folds + 1 fits */
} pols_enet_cv_out;           /* all live where b->mem says; any may be NULL */

int pols_elastic_net_cv(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_enet_cv_params *q, pols_out *out,
                        const pols_enet_cv_out *cv);

/* Two-stage least squares (instrumental variables) per group with first-stage and over-identification diagnostics (no reference
 * counterpart; linearmodels' IV2SLS / statsmodels' IV2SLS for every group of the frame in one call).
 * Fitted rows.  Per group g, the fitted rows F_g are those pols_least_squares fits -- the same null-policy filtering / zero-filling
 * and validity-mask rules, a null weight acting as 1e-24 -- with the excluded-instrument columns counted as features for every null
 * rule: a null instrument makes its row a null row, and is zero-filled where features are.  Rows are scaled by sqrt(w) (x~, z~, y~);
 * n = |F_g|.
 * Columns.  b->x_cols holds first the n_features - n_endog exogenous regressors X1, then the n_endog endogenous ones X2; the ones
 * column (add_intercept) is last and exogenous; kt = n_features + intercept, and the coefficients are in that order.  q->z_cols holds
 * the m = n_instruments excluded instruments Z2, m >= n_endog >= 1, each n_rows in the batch dtype, living where b->mem says
 * (16-byte aligned on the device).  X = [X1 | X2 | 1], Z = [X1 | 1 | Z2] with L = kt - n_endog + m columns, T = kt + m <= 31.
 * Moments and solve.  A = Z~'Z~, C = Z~'X~; Cholesky A = R R' by the static entries' f64 pivot rule (a pivot fails when
 * d^2 <= 16 dim eps A_jj); Q = R^-1 C, r = R^-1 Z~'y~, M = Q'Q (= X^'X^); b solves M b = Q'r by the same Cholesky;
 * Pi = R^-T Q, so that x^_i = Pi'z~_i.
 * Residuals.  e~_i = y~_i - x~_i'b with the ACTUAL regressors; RSS = sum e~_i^2, summed over the rows and not taken from the moments.
 * Covariance, q->cov_type.  POLS_COV_NONROBUST: V = sigma2 M^-1, sigma2 = RSS / df.  POLS_COV_HC0: V = M^-1 (sum e~_i^2 x^_i x^_i') M^-1.
 * POLS_COV_HC1: that x n / df.  Anything else is POLS_ERR_INVALID.  small_sample = 1: df = n - kt and p-values are two-sided
 * Student-t(df); small_sample = 0: df = n and p-values are two-sided normal.  se_j = sqrt(V_jj), t_j = b_j / se_j.  sigma2 is RSS / df
 * for every cov_type.
 * Diagnostics, all from the moments.  For endogenous column j, with q the column of Q that belongs to x2j: RSS_u = x~2j'x~2j - q'q;
 * D = sum of q_l^2 over the rows of Q that belong to Z2 (Z2 is last in Z, so D is the drop in the first stage's RSS from adding the
 * excluded instruments); first_stage_f[j] = (D / m) / (RSS_u / (n - L)); partial_r2[j] = D / (D + RSS_u).  Sargan's statistic
 * S = n |r - Q b|^2 / RSS, sargan_p its chi2(m - n_endog) upper tail; both are NaN when m = n_endog.
 * Outputs.  out->pred = x_i'b from the actual x, out->resid = y - pred, both unscaled, with every row predicted or masked exactly as
 * pols_least_squares does for the policy ("drop" also masks the rows with a null instrument).
 * out->status per group: POLS_GROUP_EMPTY for n = 0 (zero coefficients, everything else NaN); POLS_GROUP_BAD_DOF for 0 < n <= L
 * (everything NaN); POLS_GROUP_FALLBACK with everything NaN when A or M has no factorisation (collinear instruments, or the rank
 * condition fails) or any moment is not finite under "ignore"; otherwise POLS_GROUP_OK.  n_obs = n in every case.
 * All arithmetic is f64 on the inputs' values, for f32 batches too; coef / pred / resid are in the batch dtype, everything else is
 * f64.  No floating-point atomics, every sum in a fixed order: two runs are bit-identical, HOST and DEVICE batches agree bit for bit.
 * Groups may have any length.  When none of se / t_values / p_values / cov / sigma2 / sargan / sargan_p is asked for, the columns are
 * read once (and once more for pred / resid).
 * From pols_ols_params only null_policy is read.  POLS_ERR_INVALID: alpha != 0, positive, or has_l1_ratio with l1_ratio > 0;
 * n_endog < 1, n_endog > n_features, n_instruments < n_endog, a NULL instrument pointer; an unknown cov_type or null policy; a
 * validity mask without a drop-family policy.  POLS_ERR_UNSUPPORTED: T > 31.  There is no Arrow twin and no sharded entry. */
typedef struct pols_iv_params {
    int32_t n_endog;            /* the LAST n_endog of b->x_cols are endogenous  */
    const void *const *z_cols;  /* n_instruments excluded instruments            */
    int32_t n_instruments;
    int32_t cov_type;           /* POLS_COV_NONROBUST / POLS_COV_HC0 / POLS_COV_HC1 */
    int32_t small_sample;       /* non-zero: df = n - kt and Student-t p-values  */
} pols_iv_params;

/* n_endog = 0, z_cols = NULL, n_instruments = 0, cov_type = POLS_COV_NONROBUST, small_sample = 1 */
void pols_iv_params_default(pols_iv_params *q);

typedef struct pols_iv_out {
    double  *se;                /* n_groups x kt                                 */
    double  *t_values;          /* n_groups x kt                                 */
    double  *p_values;          /* n_groups x kt                                 */
    double  *cov;               /* n_groups x kt x kt, row-major: V              */
    double  *sigma2;            /* n_groups: RSS / df                            */
    double  *first_stage_f;     /* n_groups x n_endog                            */
    double  *partial_r2;        /* n_groups x n_endog                            */
    double  *sargan;            /* n_groups                                      */
    double  *sargan_p;          /* n_groups                                      */
    int64_t *n_obs;             /* n_groups: fitted rows                         */
} pols_iv_out;                  /* all live where b->mem says; any may be NULL */

int pols_iv2sls(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_iv_params *q, pols_out *out,
                const pols_iv_out *r);

/* AR(1) feasible generalised least squares per group: Cochrane-Orcutt / Prais-Winsten (no reference counterpart; statsmodels' GLSAR,
 * Stata's prais / prais, corc and R's prais / orcutt for every group of the frame in one call).  Everything below is per group g.
 * Rows and columns.  The rows in frame order are t = 1..n: this is TIME order, and the caller sorts.  z_t = (x_t1 .. x_tk, 1 if
 * add_intercept, y_t), kt = n_features + intercept, T = kt + 1.  All arithmetic is f64 on the inputs' values, for f32 batches too.
 * Null policies.  "ignore": the values as they are.  "zero": nulls are filled exactly as pols_least_squares does, and every row is
 * fitted.  A drop-family policy on a batch that is not null_free, or with a validity mask, is POLS_ERR_UNSUPPORTED (the lag partner
 * across a gap is not built); a null_free batch under any policy runs as "ignore".  b->weights != NULL is POLS_ERR_UNSUPPORTED.
 * Transformed model at rho.  For t = 2..n the transformed row is z*_t = z_t - rho z_{t-1}; POLS_AR1_PRAIS_WINSTEN adds
 * z*_1 = sqrt(1 - rho^2) z_1.  n* = n - 1 (Cochrane-Orcutt) or n (Prais-Winsten) transformed rows.  The ones column is transformed
 * like any other, so the intercept stays on the original scale.  With S = sum_{1..n} z z', C = sum_{t=2..n} z_t z_{t-1}',
 * S_1 = S - z_1 z_1' and S_n = S - z_n z_n':  A(rho) = S_1 - rho (C + C') + rho^2 S_n, plus (1 - rho^2) z_1 z_1' for Prais-Winsten.
 * b(rho) solves the X-block of A(rho) against its y-column by the static entries' f64 Cholesky (a pivot fails when
 * d^2 <= 16 kt eps A_jj).
 * Iteration.  rho^0 = 0, so b^0 is OLS.  Update i -> i + 1 with v = (-b^i, 1): rho^{i+1} = v'C v / v'S_n v -- the regression of e_t on
 * e_{t-1} over t = 2..n, e = y - X b^i on the ORIGINAL rows (Stata's default rhotype(regress)).  Converged when
 * |rho^{i+1} - rho^i| <= tol.  It stops on convergence, or after max_iter updates with POLS_GROUP_NOT_CONVERGED and the results still
 * returned.  n_iter is the number of updates made.  The reported coefficients are b(rho*) at the last rho (one more solve).
 * max_iter = 1 is the classical two-step estimator.
 * Reported values.  e_t = y_t - x_t'b (original scale); u_t = e_t - rho* e_{t-1} for t >= 2, u_1 = sqrt(1 - rho*^2) e_1 for
 * Prais-Winsten.  RSS* = sum u^2, summed over the rows and not taken from the moments; df = n* - kt, sigma2 = RSS* / df;
 * V = sigma2 A_xx(rho*)^-1, se_j = sqrt(V_jj), t_j = b_j / se_j, p the two-sided Student-t(df) p-value.
 * dw = sum (u_t - u_{t-1})^2 / sum u_t^2 over consecutive transformed rows; dw_ols = sum_{t>=2} (e0_t - e0_{t-1})^2 / sum_{t>=1} e0_t^2
 * with e0 = y - X b^0.  out->pred = x_t'b and out->resid = y - pred, both on the original scale.  rho = rho*.
 * out->status per group: POLS_GROUP_EMPTY for n = 0 (zero coefficients, everything else NaN, n_iter 0); POLS_GROUP_BAD_DOF for
 * n* <= kt (everything NaN); POLS_GROUP_FALLBACK with everything NaN when a pivot fails in any solve, a moment is not finite,
 * v'S_n v is not positive and finite, or |rho^{i+1}| >= 1 (n_iter: the updates made until then); POLS_GROUP_NOT_CONVERGED;
 * otherwise POLS_GROUP_OK.  n_obs = n in every case.
 * coef / pred / resid are in the batch dtype, everything else is f64.  No floating-point atomics, every sum in a fixed order: two
 * runs are bit-identical, HOST and DEVICE batches agree bit for bit.  Groups may have any length.  When none of se / t_values /
 * p_values / cov / sigma2 / dw / dw_ols is asked for, the columns are read once (and once more for pred / resid).
 * From pols_ols_params only null_policy is read.  POLS_ERR_INVALID: alpha != 0, positive, or has_l1_ratio with l1_ratio > 0; an
 * unknown method, max_iter < 1, tol not positive and finite; an unknown null policy; a validity mask without a drop-family policy.
 * POLS_ERR_UNSUPPORTED: more than 31 columns incl. the intercept, and the two cases above.  There is no Arrow twin and no sharded
 * entry. */
enum { POLS_AR1_COCHRANE_ORCUTT = 0, POLS_AR1_PRAIS_WINSTEN = 1 };

typedef struct pols_glsar_params {
    int32_t method;             /* POLS_AR1_*                                    */
    int32_t max_iter;           /* updates of rho at the most, >= 1              */
    double  tol;                /* on |rho^{i+1} - rho^i|, positive and finite   */
} pols_glsar_params;

/* method = POLS_AR1_PRAIS_WINSTEN, max_iter = 100, tol = 1e-6 (Stata's prais) */
void pols_glsar_params_default(pols_glsar_params *q);

typedef struct pols_glsar_out {
    double  *se;                /* n_groups x kt                                 */
    double  *t_values;          /* n_groups x kt                                 */
    double  *p_values;          /* n_groups x kt                                 */
    double  *cov;               /* n_groups x kt x kt, row-major: V              */
    double  *sigma2;            /* n_groups: RSS* / df                           */
    double  *rho;               /* n_groups: rho*                                */
    double  *dw;                /* n_groups: Durbin-Watson of the transformed residuals */
    double  *dw_ols;            /* n_groups: Durbin-Watson of the OLS residuals  */
    int32_t *n_iter;            /* n_groups: rho updates made                    */
    int64_t *n_obs;             /* n_groups: n                                   */
} pols_glsar_out;               /* all live where b->mem says; any may be NULL */

int pols_glsar(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_glsar_params *q, pols_out *out,
               const pols_glsar_out *r);

/* Regression that absorbs one categorical effect inside every group -- the "within" estimator (no reference counterpart; Stata's
 * areg / xtreg, fe and linearmodels' PanelOLS(entity_effects=True) for every group of the frame in one call, without a dummy column
 * per category).  Everything below is per group g.
 * Fitted rows.  F_g are the rows pols_least_squares fits under the policy -- the same null rules, validity-mask rule and null-weight
 * rule (1e-24); n = |F_g|.  q->ids holds one 64-bit id per row in the batch's row order, living where b->mem says; ids follow their
 * rows through the policy and carry no nulls.
 * Categories.  The distinct ids among F_g; C is their number.  A category with one fitted row counts in C and contributes a zero row.
 * Within transform, over the k = n_features user columns only (the ones column is never part of the fit): W_c = sum_{i in c} w_i
 * (w = 1 without weights), xbar_c = sum w_i x_i / W_c, ybar_c likewise; x~_i = sqrt(w_i) (x_i - xbar_c(i)), y~_i likewise.  The means
 * are computed first and the moments are those of the demeaned rows (never raw moments minus a per-category correction).
 * Solve.  A = X~'X~ = L L' by Cholesky; pivot j fails when d_j <= 16 k eps T_jj with T_jj = sum w_i x_ij^2, the RAW second moment: a
 * column that is constant inside every category up to rounding is flagged.  b = A^-1 X~'y~; e~_i = y~_i - x~_i'b; RSS = sum e~_i^2,
 * summed over the rows and not taken from the moments.
 * Effects.  a_c = ybar_c - xbar_c'b.  With add_intercept coef[kt - 1] = c0 = sum_c W_c a_c / sum_c W_c and fe_i = a_c(i) - c0;
 * without it fe_i = a_c(i).  out->pred = x_i'b + a_c(i), out->resid = y - pred, every row predicted or masked exactly as
 * pols_least_squares does for the policy; a row outside F_g whose id has no fitted row in its group gets NaN in pred, resid and fe.
 * Inference.  df = n - k - C, sigma2 = RSS / df.  POLS_COV_NONROBUST: V = sigma2 A^-1, p two-sided Student-t(df).
 * POLS_COV_CLUSTER (clustered on the ids): s_c = sum_{i in c} e~_i x~_i, V = q A^-1 (sum_c s_c s_c') A^-1 with
 * q = C / (C - 1) (n - 1) / (n - k - 1) -- the nested-cluster convention: the absorbed effects are not charged again --, p two-sided
 * Student-t(C - 1); NaN when C < 2 or n - k - 1 <= 0.  se_j = sqrt(V_jj), t_j = b_j / se_j; the intercept's se / t / p are NaN.
 * r2_within = 1 - RSS / sum y~_i^2; r2 = 1 - RSS / sum w_i (y_i - ybar_w)^2 (the total sum of squares is formed as the within sum
 * plus sum_c W_c (ybar_c - ybar_w)^2).
 * out->status: POLS_GROUP_EMPTY for n = 0 (zero coefficients, everything else NaN); POLS_GROUP_BAD_DOF for df <= 0 (everything NaN);
 * POLS_GROUP_FALLBACK with everything NaN when a pivot fails or a moment is not finite; otherwise POLS_GROUP_OK.  n_obs and
 * n_categories are written in every case.
 * All arithmetic is f64 on the inputs' values, for f32 batches too; coef / pred / resid / fe are in the batch dtype, everything else
 * is f64.  No floating-point atomics; every sum runs in a fixed order -- a group's categories by ascending id, a category's rows by
 * position (frame order inside an id) in batches of 64 whose terms meet in a fixed tree, segments of a long group in segment order --
 * so two runs are bit-identical and HOST and DEVICE batches agree bit for bit.  Groups may have any length.  The call synchronises
 * the stream twice (the order probe, the number of categories).  When none of se / t_values / p_values / sigma2 / r2_within / r2 is
 * asked for, the residual pass is skipped.
 * From pols_ols_params only null_policy is read.  POLS_ERR_INVALID: NULL ids; n_features < 1; alpha != 0, positive, or has_l1_ratio
 * with l1_ratio > 0; a cov_type other than the two named; a validity mask without a drop-family policy; on the device, a pred / resid
 * / fe that is not 16-byte aligned.  POLS_ERR_UNSUPPORTED: kt > 31 or n_rows >= 2^31.  There is no Arrow twin and no sharded entry.
 * Not built: HC0-HC3 / HAC covariance on absorbed fits; penalised fits; rolling / recursive forms. */
typedef struct pols_absorb_params {
    const int64_t *ids;         /* one id per row, in the batch's row order, where b->mem says */
    int32_t cov_type;           /* POLS_COV_NONROBUST or POLS_COV_CLUSTER (clustered on ids)    */
} pols_absorb_params;

/* ids = NULL, cov_type = POLS_COV_NONROBUST */
void pols_absorb_params_default(pols_absorb_params *q);

typedef struct pols_absorb_out {
    double  *se;                /* n_groups x kt                                 */
    double  *t_values;          /* n_groups x kt                                 */
    double  *p_values;          /* n_groups x kt                                 */
    double  *sigma2;            /* n_groups: RSS / df                            */
    double  *r2_within;         /* n_groups                                      */
    double  *r2;                /* n_groups                                      */
    void    *fe;                /* n_rows, batch dtype: the row's effect         */
    int64_t *n_obs;             /* n_groups: fitted rows                         */
    int64_t *n_categories;      /* n_groups: C                                   */
} pols_absorb_out;              /* all live where b->mem says; any may be NULL */

int pols_least_squares_absorb(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_absorb_params *q,
                              pols_out *out, const pols_absorb_out *r);

/* Regression that absorbs TWO categorical effects inside every group -- two-way fixed effects (no reference counterpart; Stata's
 * reghdfe y x, absorb(firm year) and linearmodels' PanelOLS(entity_effects=True, time_effects=True) for every group of the frame in
 * one call, without a dummy column per category).  Everything below is per group g.  F_g, n, the weights (a null weight acts as 1e-24),
 * the null-policy rules and the validity-mask rule are exactly those of pols_least_squares_absorb above.  q->ids and q->ids2 hold one
 * 64-bit id per row each, in the batch's row order, living where b->mem says; they carry no nulls.  All arithmetic is f64 on the
 * inputs' values, for f32 batches too.
 * Categories and components.  C1 and C2 are the numbers of distinct ids of each column among F_g (a category with one fitted row
 * counts).  M is the number of connected components of the bipartite graph whose vertices are the categories and whose edges are the
 * fitted rows.  M is exact: the labels are propagated until nothing changes, whatever max_iter says.
 * Demeaning one column v (y and each of the k = n_features user columns, each on its own; never a ones column).  Start from v0, the
 * values the fit sees under the policy.  One sweep does two steps: m1_c = sum_{i in c} w_i v_i / W1_c for every id-1 category, then
 * v_i -= m1_c1(i); on the updated v, m2_d = sum_{i in d} w_i v_i / W2_d for every id-2 category, then v_i -= m2_c2(i).  The iteration
 * stops after the first sweep with max(max_c |m1_c|, max_d |m2_d|) <= tol s, where s = sqrt(sum w_i v0_i^2 / sum w_i); otherwise after
 * max_iter sweeps.  At least one sweep is made.  The column's accumulated means are a1_c(v) = the sum of m1_c over the sweeps, a2_d(v)
 * likewise.  x~_i = sqrt(w_i) v_i(final), y~ likewise.
 * Solve.  A = X~'X~ = L L' by Cholesky with the pivot rule of pols_least_squares_absorb unchanged: pivot j fails when
 * d_j <= 16 k eps T_jj, T_jj = sum w_i x_ij^2 the RAW second moment.  b = A^-1 X~'y~; e~ = y~ - X~ b; RSS = sum e~_i^2 over the rows.
 * Inference.  df = n - k - (C1 + C2 - M), sigma2 = RSS / df.  POLS_COV_NONROBUST: V = sigma2 A^-1, p two-sided Student-t(df).
 * POLS_COV_CLUSTER (clustered on ids, the first column): s_c = sum_{i in c} e~_i x~_i over the id-1 categories,
 * V = q A^-1 (sum_c s_c s_c') A^-1 with q = C1 / (C1 - 1) (n - 1) / (n - k - 1 - (C2 - M)) -- the nested convention of
 * pols_least_squares_absorb with the second effect charged like regressors --, p two-sided Student-t(C1 - 1); NaN when C1 < 2 or the
 * denominator is <= 0.  The intercept's se / t / p are NaN.  r2_within = 1 - RSS / sum y~_i^2, r2 = 1 - RSS / sum w_i (y_i - ybar_w)^2.
 * Effects and rows.  a1_c = a1_c(y) - sum_j b_j a1_c(x_j), a2_d likewise.  pred_i = x_i'b + a1_c1(i) + a2_c2(i) for every row,
 * resid = y - pred.  With add_intercept coef[kt - 1] = c0 = sum_{F_g} w_i (a1 + a2)_i / sum w_i, and fe1_i, fe2_i are each centred on
 * their own weighted mean over F_g, so that c0 + fe1 + fe2 = a1 + a2; without it fe1 = a1 and fe2 = a2.  Only the sum a1 + a2 is
 * identified: the split between the two is whatever the iteration started from zero gives (inside every component a constant can move
 * from one effect to the other).  A row outside F_g gets NaN in pred / resid / fe1 / fe2 when either of its ids has no fitted row in
 * the group, or when its two categories lie in different components; otherwise it is predicted.
 * out->status, in this precedence: POLS_GROUP_EMPTY for n = 0 (zero coefficients, everything else NaN); POLS_GROUP_BAD_DOF for
 * df <= 0 (everything NaN); POLS_GROUP_FALLBACK with everything NaN when a pivot fails or a moment is not finite;
 * POLS_GROUP_NOT_CONVERGED when a column made max_iter sweeps without the stop rule firing (the result is still returned, as pols_rlm
 * and pols_glm do); otherwise POLS_GROUP_OK.  n_iter[g] is the largest sweep count among the k + 1 columns.  n_obs, n_categories,
 * n_categories2, n_components and n_iter are written in every case.  At the default tol a column that is an exact sum
 * f(id1) + g(id2) is demeaned to rounding noise and flagged by the pivot rule; with a loose tol what the iteration leaves may pass it.
 * Determinism as pols_least_squares_absorb: no floating-point atomics; a category's rows are summed by position (frame order inside an
 * id) in batches of 64 whose terms meet in a fixed tree, the batches in position order; reruns are bit-identical, and HOST and DEVICE
 * batches agree bit for bit.  A group's result depends on nothing outside the group.  Groups may have any length: one workgroup per
 * (group, column) iterates with its column in LDS when the group has at most 11 684 rows (7 435 when the store carries weights: a
 * weights column, or a policy that can take rows out of the fit) -- 14 n + 4 | 22 n + 4 bytes of the 163 584 a launch may ask for --
 * and on a global f64 scratch of (k + 1) x n_rows otherwise, with the same bits on a group that fits both.  The option
 * POLS_ABSORB2_ROUTE=global sends every group to the scratch form (resident / unset: LDS wherever the group fits).  The call
 * synchronises the stream three times (the two order probes, the category counts).
 * From pols_ols_params only null_policy is read.  POLS_ERR_INVALID: NULL ids or ids2; max_iter < 1; a tol that is not positive and
 * finite; n_features < 1; alpha != 0, positive, or has_l1_ratio with l1_ratio > 0; a cov_type other than the two named; a validity
 * mask without a drop-family policy; on the device, a pred / resid / fe1 / fe2 that is not 16-byte aligned.  POLS_ERR_UNSUPPORTED:
 * kt > 31 or n_rows >= 2^31.  There is no Arrow twin and no sharded entry.
 * Not built: three or more absorbed ids; acceleration of the iteration (conjugate gradient, symmetric Kaczmarz); a multi-workgroup
 * form for one very long column; HC / HAC and two-way cluster covariance on absorbed fits; Arrow and sharded twins. */
typedef struct pols_absorb2_params {
    const int64_t *ids;         /* first id per row (the clustering of POLS_COV_CLUSTER), where b->mem says */
    const int64_t *ids2;        /* second id per row                                                         */
    int32_t cov_type;           /* POLS_COV_NONROBUST or POLS_COV_CLUSTER                                    */
    int32_t max_iter;           /* sweeps per column at the most, >= 1                                       */
    double  tol;                /* stop rule, relative to the column's root mean square; positive and finite */
} pols_absorb2_params;

/* ids = NULL, ids2 = NULL, cov_type = POLS_COV_NONROBUST, max_iter = 10000, tol = 1e-10 */
void pols_absorb2_params_default(pols_absorb2_params *q);

typedef struct pols_absorb2_out {
    double  *se;                /* n_groups x kt                                 */
    double  *t_values;          /* n_groups x kt                                 */
    double  *p_values;          /* n_groups x kt                                 */
    double  *sigma2;            /* n_groups: RSS / df                            */
    double  *r2_within;         /* n_groups                                      */
    double  *r2;                /* n_groups                                      */
    void    *fe1;               /* n_rows, batch dtype: the row's first effect   */
    void    *fe2;               /* n_rows, batch dtype: the row's second effect  */
    int64_t *n_obs;             /* n_groups: fitted rows                         */
    int64_t *n_categories;      /* n_groups: C1                                  */
    int64_t *n_categories2;     /* n_groups: C2                                  */
    int64_t *n_components;      /* n_groups: M                                   */
    int32_t *n_iter;            /* n_groups: most sweeps among the k + 1 columns */
} pols_absorb2_out;             /* all live where b->mem says; any may be NULL */

int pols_least_squares_absorb2(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_absorb2_params *q,
                               pols_out *out, const pols_absorb2_out *r);

/* Random-effects panel regression with the Hausman test inside every group (no reference counterpart; Stata's xtreg, re followed by
 * hausman, linearmodels' RandomEffects and BetweenOLS, for every group of the frame in one call).  Everything below is per group g.
 * Fitted rows, ids and categories.  Exactly as pols_least_squares_absorb: the same null policies, validity-mask rule and id rules.  n is
 * the number of fitted rows, C the number of categories, T_c the fitted rows of category c, k = n_features, kc = kt = k + 1 with
 * add_intercept (the intercept is the last coefficient).  Weights are not built: a batch with weights is refused.
 * 1. Within.  The fit of pols_least_squares_absorb unchanged: b_w, A_w = X~'X~, X~'y~ and RSS_w, summed over the rows;
 * df_w = n - k - C, sigma2_e = RSS_w / df_w.
 * 2. Between.  zbar_c = (xbar_c, 1) with the intercept, xbar_c without; the regression is unweighted over the categories:
 * B = sum_c zbar_c zbar_c', b_b = B^-1 sum_c zbar_c ybar_c by Cholesky, pivot j fails when d_j <= 16 kc eps sum_c zbar_cj^2;
 * RSS_b = sum_c (ybar_c - zbar_c'b_b)^2, summed over the table of category means and not taken from the moments; df_b = C - kc.
 * 3. Variance components (Swamy-Arora, Stata's default for unbalanced panels).  Tbar = C / sum_c (1 / T_c),
 * sigma2_u = max(0, RSS_b / df_b - sigma2_e / Tbar), rho = sigma2_u / (sigma2_u + sigma2_e),
 * theta_c = 1 - sqrt(sigma2_e / (sigma2_e + T_c sigma2_u)).
 * 4. GLS.  q_c = T_c (1 - theta_c)^2; M = embed(A_w) + sum_c q_c zbar_c zbar_c', v = embed(X~'y~) + sum_c q_c zbar_c ybar_c,
 * b = M^-1 v by Cholesky, pivot j fails when d_j <= 16 kc eps T_jj with T_jj the raw second moment sum x_ij^2 (n for the intercept).
 * "embed" puts the k x k within block into the leading corner and zeros into the intercept's row and column.  With
 * x*_i = x_i - theta_c xbar_c = x~_i + (1 - theta_c) xbar_c the cross terms vanish inside a category, so M = X*'X* and v = X*'y*: the
 * quasi-demeaned columns are never formed.
 * 5. Residual sum.  RSS = sum_i (y~_i - x~_i'b_1..k)^2 + sum_c q_c (ybar_c - zbar_c'b)^2, the first term from the rows and the second
 * from the table; df = n - kc, sigma2 = RSS / df.
 * 6. Inference.  V = sigma2 M^-1, se_j = sqrt(V_jj), t_j = b_j / se_j, p two-sided Student-t(df), the intercept included.
 * 7. Hausman.  d = b_w - b_1..k, D = sigma2_e (A_w^-1 - (M^-1)_1..k,1..k) -- sigma2_e on both sides, which makes D positive
 * semi-definite by construction --, H = d'D^-1 d by Cholesky of D, hausman_p = Q(k / 2, H / 2), the upper tail of chi2(k).  Both are NaN
 * when a pivot of D is not positive; the group's status is unaffected.
 * 8. Effects.  u_c = T_c sigma2_u / (T_c sigma2_u + sigma2_e) (ybar_c - zbar_c'b).
 * 9. Row outputs.  out->pred = z_i'b with no effect added, out->resid = y - pred, every row predicted or masked exactly as
 * pols_least_squares does for the policy.  effects and theta hold u_c(i) and theta_c(i) per row in the batch dtype; NaN for a row whose
 * id has no fitted row in its group.  out->coef is b.
 * out->status: POLS_GROUP_EMPTY for n = 0 (zero coefficients, everything else NaN); POLS_GROUP_BAD_DOF for df_w <= 0 or df_b <= 0
 * (everything NaN); POLS_GROUP_FALLBACK with everything NaN when any of the three pivots fails or a sum is not finite; otherwise
 * POLS_GROUP_OK.  n_obs and n_categories are written in every case.
 * All arithmetic is f64 on the inputs' values, for f32 batches too.  No floating-point atomics; every sum runs in a fixed order.  The
 * within sums are those of pols_least_squares_absorb.  A sum over the table of a group runs over its categories by ascending id: an
 * entry of B or M (packed triangles of kc + 1 columns, ybar the last, E = (kc + 1)(kc + 2) / 2 entries) in P = 256 / E interleaved
 * partitions (P = 1 beyond 256 entries), partition p over categories p, p + P, .., the partitions added in order and the within moment
 * last; a scalar (RSS_b, sum 1 / T_c, the table's part of RSS) in 256 interleaved partitions that meet in a fixed tree.  The row term of
 * RSS is summed as RSS_w is.  Results are bit-identical run to run, between HOST and DEVICE batches, and between the two routes of the
 * table kernel: a group whose rows of the table fit a workgroup's LDS is held there, any other is read from global memory
 * (POLS_RANDOM_EFFECTS_ROUTE=global sends every group there).  The call synchronises the stream twice (the order probe, the category
 * counts).  When none of se / t_values / p_values is asked for, the second residual pass is skipped.
 * From pols_ols_params only null_policy is read.  POLS_ERR_INVALID: NULL ids; n_features < 1; alpha != 0, positive, or has_l1_ratio
 * with l1_ratio > 0; a validity mask without a drop-family policy; on the device, a pred / resid / effects / theta that is not 16-byte
 * aligned.  POLS_ERR_UNSUPPORTED: weights; kt > 31 or n_rows >= 2^31.  There is no Arrow twin and no sharded entry.
 * Not built: weights; time effects or two-way random effects; robust or clustered covariance; other variance-component estimators;
 * the Mundlak / robust Hausman form; Stata's three R2. */
typedef struct pols_random_effects_params {
    const int64_t *ids;         /* one entity id per row, in the batch's row order, where b->mem says */
} pols_random_effects_params;

/* ids = NULL */
void pols_random_effects_params_default(pols_random_effects_params *q);

typedef struct pols_random_effects_out {
    double  *se;                /* n_groups x kt                                 */
    double  *t_values;          /* n_groups x kt                                 */
    double  *p_values;          /* n_groups x kt                                 */
    double  *coef_between;      /* n_groups x kt: b_b                            */
    double  *coef_within;       /* n_groups x n_features: b_w                    */
    double  *sigma2_e;          /* n_groups                                      */
    double  *sigma2_u;          /* n_groups                                      */
    double  *rho;               /* n_groups                                      */
    double  *hausman;           /* n_groups: H                                   */
    double  *hausman_p;         /* n_groups                                      */
    void    *effects;           /* n_rows, batch dtype: the row's u_c            */
    void    *theta;             /* n_rows, batch dtype: the row's theta_c        */
    int64_t *n_obs;             /* n_groups: fitted rows                         */
    int64_t *n_categories;      /* n_groups: C                                   */
} pols_random_effects_out;      /* all live where b->mem says; any may be NULL */

int pols_random_effects(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_random_effects_params *q,
                        pols_out *out, const pols_random_effects_out *r);

/* ---- group-key ingestion: `.over(key)` / `group_by(key)` ------------------------------------------------------------
 * The reference's plugin functions never see a key column: Polars partitions the frame on the host and calls them once per
 * group (README.md:19, README.md:57 and :91 `.over("group")`, tests/test_ols.py:110, :384, :860).  The batched entries
 * above take the whole frame with rows sorted by group, so the host needs that partitioning; these entries do it where the
 * columns live.  A pols_layout holds, for one key column of one frame: the stable permutation `order` (sorted position i
 * holds frame row order[i]; rows of a group keep their frame order, which the recursive / rolling models depend on), the
 * groups' offsets and keys (ascending).  Keys are 64-bit integers (the host hashes / dictionary-encodes anything else, as
 * Polars does for its own group-by).  Fewer than 2^32 rows. */
typedef struct pols_layout pols_layout;
/* keys: n_rows int64 where `mem` says.  Synchronises the context's stream (the group count comes back to the host). */
int pols_layout_create(pols_ctx *ctx, const int64_t *keys, int64_t n_rows, int mem, pols_layout **out);
void pols_layout_destroy(pols_layout *layout);
int64_t pols_layout_n_rows(const pols_layout *layout);
int64_t pols_layout_n_groups(const pols_layout *layout);
/* 1 when the key column was already non-decreasing: take / untake are copies, callers may skip them and pass the frame's
 * own columns. */
int pols_layout_is_identity(const pols_layout *layout);
/* host arrays owned by the layout: n_groups + 1 offsets (pass as pols_batch.group_offsets) and n_groups keys */
const int64_t *pols_layout_group_offsets(const pols_layout *layout);
const int64_t *pols_layout_group_keys(const pols_layout *layout);
/* frame order -> group order: dst[c][i] = src[c][order[i]] for n_cols columns whose elements are element_bytes wide: 1
 * (validity bytes), 4 or 8 (f32 / f64 columns), or any other multiple of 4 for row-major tables moved a row at a time
 * (an [n_rows, k] coefficient table is one "column" of k * sizeof(T)-byte elements).  src != dst.  `mem` says where BOTH tables' columns live (host columns are staged through the device). */
int pols_layout_take(pols_ctx *ctx, pols_layout *layout, int element_bytes, const void *const *src_cols, void *const *dst_cols,
                     int32_t n_cols, int mem);
/* group order -> frame order: dst[c][order[i]] = src[c][i]  (predictions / residuals / per-row coefficients back onto the
 * frame, like the Series `.over` returns). */
int pols_layout_untake(pols_ctx *ctx, pols_layout *layout, int element_bytes, const void *const *src_cols, void *const *dst_cols,
                       int32_t n_cols, int mem);
/* out[r] = index (into group_keys / a coefficient table) of the group frame row r belongs to: what broadcasts a per-group
 * coefficient struct over the frame (mode="coefficients" under `.over`, README.md:91). */
int pols_layout_row_groups(pols_ctx *ctx, pols_layout *layout, int64_t *out, int mem);

/* ---- Arrow C Data Interface entry: what the reference's plugin functions do AROUND the solver ---------------------------------
 * `#[polars_expr] fn least_squares(inputs: &[Series], kwargs)` / `least_squares_coefficients` (src/expressions.rs:390-446) receive
 * their Series over the Arrow C Data Interface (one ArrowArray per chunk: values + optional validity BITMAP + element offset),
 * cast them to Float64 with nulls -> NaN and rechunk (convert_polars_to_ndarray :66-103), and return a Series the same way
 * (Float64 with a validity mask :145-158, or a struct of per-feature coefficients with NaN -> null :114-143).  This entry takes
 * the arrays exactly as Polars holds them -- any numeric primitive type, null bitmaps, sliced (offset != 0) and multi-chunk
 * columns -- and hands back a released-by-callback ArrowArray / ArrowSchema pair.  The structs below are the interface's own ABI
 * (https://arrow.apache.org/docs/format/CDataInterface.html); the guard is the one every implementation uses. */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
struct ArrowSchema {
    const char *format;
    const char *name;
    const char *metadata;
    int64_t flags;
    int64_t n_children;
    struct ArrowSchema **children;
    struct ArrowSchema *dictionary;
    void (*release)(struct ArrowSchema *);
    void *private_data;
};
struct ArrowArray {
    int64_t length;
    int64_t null_count;
    int64_t offset;
    int64_t n_buffers;
    int64_t n_children;
    const void **buffers;
    struct ArrowArray **children;
    struct ArrowArray *dictionary;
    void (*release)(struct ArrowArray *);
    void *private_data;
};
#endif

typedef struct {
    const struct ArrowSchema *schema;         /* format: g f l L i I s S c C (what the reference can cast to Float64) */
    const struct ArrowArray *const *chunks;   /* the Series' chunks, in order; host memory; borrowed for the duration of the call */
    int32_t n_chunks;
} pols_arrow_column;

typedef enum { POLS_MODE_PREDICTIONS = 0, POLS_MODE_RESIDUALS = 1, POLS_MODE_COEFFICIENTS = 2 } pols_output_mode;

/* target / features / weights: inputs[0], inputs[1..] and the sample_weights expression of polars_ols/least_squares.py:163-239
 * (sqrt(w) scaling, the "const" column and the 1/sqrt(w) un-scaling are fused, as in pols_least_squares).  group_offsets NULL
 * = one group holding every row (the per-group call a plugin receives); otherwise rows sorted by group as in pols_batch.
 * Every input Float32 -> computed and returned in f32; anything else -> f64 (the reference's Float64).
 * out / out_schema: caller-allocated structs, filled in; the caller releases them through their `release` callbacks.
 *   predictions / residuals: a primitive array of n_rows values named after the target; nulls where null_policy "drop" masks
 *                            the rows it left out of the fit (residuals: also where the target is null)
 *   coefficients:            a struct array "coefficients" of n_groups rows, one field per feature (+ "const"), NaN -> null */
int pols_least_squares_arrow(pols_ctx *ctx, const pols_arrow_column *target, const pols_arrow_column *features, int32_t n_features,
                             const pols_arrow_column *weights, const int64_t *group_offsets, int64_t n_groups, int32_t add_intercept,
                             const pols_ols_params *p, int32_t mode, struct ArrowArray *out, struct ArrowSchema *out_schema);

/* The other seven plugin functions (src/expressions.rs:468-741), same conventions: columns as Polars holds them in, a
 * released-by-callback ArrowArray / ArrowSchema pair out; group_offsets NULL = the per-group call; all inputs Float32 -> f32.
 *
 * least_squares_statistics (ex.rs:448-509): a struct array "statistics" with ONE row per group and the fields of
 * statistics_struct_dtype (:448-466): r2, mae, mse (Float64), feature_names (list<str>), coefficients, standard_errors,
 * t_values, p_values (list<Float64>); lists are Arrow large lists ("+L") of large strings ("U") / Float64.  A group whose
 * degrees of freedom are <= 0 fails the call with POLS_ERR_PANIC like the reference's assert (src/statistics.rs:131-134). */
int pols_least_squares_statistics_arrow(pols_ctx *ctx, const pols_arrow_column *target, const pols_arrow_column *features,
                                        int32_t n_features, const pols_arrow_column *weights, const int64_t *group_offsets,
                                        int64_t n_groups, int32_t add_intercept, const pols_ols_params *p, struct ArrowArray *out,
                                        struct ArrowSchema *out_schema);
/* pols_least_squares_statistics_arrow with robust standard errors (pols_least_squares_statistics_robust): the same struct schema,
 * `cov` after `p`. */
int pols_least_squares_statistics_robust_arrow(pols_ctx *ctx, const pols_arrow_column *target, const pols_arrow_column *features,
                                               int32_t n_features, const pols_arrow_column *weights, const int64_t *group_offsets,
                                               int64_t n_groups, int32_t add_intercept, const pols_ols_params *p,
                                               const pols_cov_params *cov, struct ArrowArray *out, struct ArrowSchema *out_schema);
/* pols_least_squares_statistics_arrow with cluster-robust standard errors (pols_least_squares_statistics_cluster): the same struct
 * schema.  ids[0] (and ids[1] for POLS_COV_CLUSTER2) are integer columns (formats l L i I s S c C), one row per target row; a null
 * id is POLS_ERR_INVALID.  cl->ids and cl->n_clusters are ignored. */
int pols_least_squares_statistics_cluster_arrow(pols_ctx *ctx, const pols_arrow_column *target, const pols_arrow_column *features,
                                                int32_t n_features, const pols_arrow_column *weights, const int64_t *group_offsets,
                                                int64_t n_groups, int32_t add_intercept, const pols_ols_params *p,
                                                const pols_cluster_params *cl, const pols_arrow_column *ids, int32_t n_ids,
                                                struct ArrowArray *out, struct ArrowSchema *out_schema);
/* pols_least_squares_influence over Arrow columns: a struct array "influence" of n_rows rows whose fields are the per-row arrays named
 * in `fields` (a mask of POLS_INFL_* bits; 0 = all), in pols_influence_out's order and under its names, Float32 when every input is
 * Float32, else Float64; a null stands where the plain entry writes NaN for "not defined". */
int pols_least_squares_influence_arrow(pols_ctx *ctx, const pols_arrow_column *target, const pols_arrow_column *features,
                                       int32_t n_features, const pols_arrow_column *weights, const int64_t *group_offsets,
                                       int64_t n_groups, int32_t add_intercept, const pols_ols_params *p,
                                       const pols_influence_params *q, uint32_t fields, struct ArrowArray *out,
                                       struct ArrowSchema *out_schema);
/* multi_target_least_squares (ex.rs:511-591): `targets` is the STRUCT Series of inputs[0] (format "+s", one numeric field per
 * target; a null struct row is a null in every field); out: a struct array "predictions" of n_rows rows with the targets' field
 * names (multi_target_struct_dtype, :511-519), NaN -> null.  Residuals are the caller's `target - predictions`
 * (polars_ols/least_squares.py:236-239). */
int pols_multi_target_least_squares_arrow(pols_ctx *ctx, const pols_arrow_column *targets, const pols_arrow_column *features,
                                          int32_t n_features, const pols_arrow_column *weights, const int64_t *group_offsets,
                                          int64_t n_groups, int32_t add_intercept, const pols_ols_params *p, struct ArrowArray *out,
                                          struct ArrowSchema *out_schema);
/* recursive_least_squares / recursive_least_squares_coefficients (ex.rs:593-646) and rolling_least_squares /
 * rolling_least_squares_coefficients (:648-701); mode POLS_MODE_PREDICTIONS: a primitive array named after the target, null where
 * the validity mask of the null policy masks the row (make_predictions with is_valid, :640-645) or no estimate exists yet;
 * POLS_MODE_COEFFICIENTS: a struct array "coefficients" with ONE ROW PER INPUT ROW, one field per feature (+ "const"), NaN -> null.
 * Quirk kept: the reference's prediction form of RLS ignores initial_state_mean (ex.rs:636) -- pass NULL for it there. */
int pols_recursive_least_squares_arrow(pols_ctx *ctx, const pols_arrow_column *target, const pols_arrow_column *features,
                                       int32_t n_features, const pols_arrow_column *weights, const int64_t *group_offsets,
                                       int64_t n_groups, int32_t add_intercept, const pols_rls_params *p, int32_t mode,
                                       struct ArrowArray *out, struct ArrowSchema *out_schema);
int pols_rolling_least_squares_arrow(pols_ctx *ctx, const pols_arrow_column *target, const pols_arrow_column *features,
                                     int32_t n_features, const pols_arrow_column *weights, const int64_t *group_offsets,
                                     int64_t n_groups, int32_t add_intercept, const pols_rolling_params *p, int32_t mode,
                                     struct ArrowArray *out, struct ArrowSchema *out_schema);
/* predict (ex.rs:706-741): `coefficients` is the coefficients STRUCT Series of inputs[0] -- one row per input row (what Polars
 * broadcasts / joins it to), n_features (+ 1 with add_intercept: the pl.lit(1.0) "const" feature of least_squares.py:479-483)
 * numeric fields; null_policy is one of ignore / zero / drop (least_squares.py:474): features are zero-filled unless "ignore"
 * (:725), "drop" nulls the rows with a null anywhere (:732-738).  out: a primitive array named `name` (NULL / "" -> "predictions"). */
int pols_predict_arrow(pols_ctx *ctx, const pols_arrow_column *coefficients, const pols_arrow_column *features, int32_t n_features,
                       int32_t add_intercept, int32_t null_policy, const char *name, struct ArrowArray *out,
                       struct ArrowSchema *out_schema);

/* ---- more than one GPU ------------------------------------------------------------------------------------------------
 * Groups are independent in the reference -- every plugin call sees one group's rows, nothing in src/least_squares.rs carries
 * state across groups, and Polars runs the calls concurrently on its rayon pool (README.md:19) -- so the data path has NO
 * collective: each GPU owns a contiguous range of groups (balanced by rows) and runs the same entries on its shard through its
 * own pols_ctx.  The one exchange step is what Polars does when it concatenates the per-group outputs: re-assembling an output
 * column.  These entries do that over RCCL / xGMI.  RCCL is bound at run time (librccl.so.1; an instance the process already
 * holds is reused), so single-GPU callers never load it.
 *
 *   one process per GPU (MPI / torch.distributed launch):  rank 0 calls pols_comm_unique_id, ships the 128 bytes to every rank
 *       out of band, every rank calls pols_comm_create with its own context.
 *   one process, several GPUs (what a Polars plugin process is):  pols_create per device, then ONE pols_comm_create_all; the
 *       per-device collective calls of one exchange are bracketed by pols_comm_group_begin / _end (or issued from one host
 *       thread per device).
 * Collectives are asynchronous on the context's stream (ordered behind the kernels that produced `local`). */
typedef struct pols_comm pols_comm;
#define POLS_COMM_ID_BYTES 128
/* bounds_out[0 .. world_size]: rank r owns groups [bounds_out[r], bounds_out[r + 1]); boundary r is the first group boundary whose
 * cumulative row count reaches r / world_size of the rows.  A pure function of the offsets: no communication needed to agree. */
int pols_partition_groups(const int64_t *group_offsets, int64_t n_groups, int world_size, int64_t *bounds_out);
int pols_comm_unique_id(void *id_out /* POLS_COMM_ID_BYTES */);
int pols_comm_create(pols_ctx *ctx, const void *id, int world_size, int rank, pols_comm **out);
int pols_comm_create_all(pols_ctx *const *ctxs, int n, pols_comm **out /* n communicators, rank i on ctxs[i]'s device */);
void pols_comm_destroy(pols_comm *comm);
int pols_comm_world_size(const pols_comm *comm);
int pols_comm_rank(const pols_comm *comm);
/* What RCCL itself says about this communicator -- not what the caller passed to pols_comm_create: the rank count and rank the library
 * reports (ncclCommCount / ncclCommUserRank), the HIP device it is bound to (ncclCommCuDevice) with its PCI bus id, and the library's
 * version code (ncclGetVersion).  A measurement line that carries these proves the collective saw N ranks on N different devices. */
typedef struct pols_comm_info {
    int32_t nranks_seen, rank_seen, device, rccl_version;
    char pci_bus_id[32];
} pols_comm_info;
int pols_comm_query(const pols_comm *comm, pols_comm_info *out);
int pols_comm_group_begin(void);
int pols_comm_group_end(void);
/* Every rank receives all rows, in rank order (= group order, the shards being contiguous ranges): `local` holds counts[rank]
 * rows of row_bytes bytes (a [groups x k] coefficient table: row_bytes = k * sizeof(element)), `out` sum(counts) rows; both
 * DEVICE.  One ncclAllGather when every shard has the same size, otherwise one grouped broadcast per owner (all-gatherv). */
int pols_comm_allgather_rows(pols_comm *comm, const void *local, const int64_t *counts, int64_t row_bytes, void *out);
/* Per-row outputs (predictions / residuals) to ONE root, in frame order: grouped ncclSend / ncclRecv -- over point-to-point xGMI
 * the root pulls from its peers over distinct links at once, where a ring all-gather would be bound by one link. */
int pols_comm_gather_rows(pols_comm *comm, const void *local, const int64_t *counts, int64_t row_bytes, int root, void *out_on_root);

/* One process, several GPUs -- the form a Polars plugin process takes: the frame sits in HOST memory (b->mem must be POLS_MEM_HOST),
 * ctxs[0 .. n) are contexts on n devices.  The groups are cut into n contiguous ranges balanced by rows (pols_partition_groups),
 * range r is staged to and solved on ctxs[r]'s device from its own host thread, exactly as pols_least_squares would, and the outputs
 * named in `o` are re-assembled according to out_mem:
 *   POLS_MEM_HOST    o's pointers are host arrays for the WHOLE frame; every device copies its slice into them (no collective;
 *                    comms may be NULL);
 *   POLS_MEM_DEVICE  o's pointers are buffers on ctxs[0]'s device for the whole frame: the coefficient table is all-gathered
 *                    (pols_comm_allgather_rows), predictions / residuals / status are gathered to device 0 (pols_comm_gather_rows)
 *                    over RCCL / xGMI; comms[r] must be rank r of a world of n (pols_comm_create_all).  Returns when device 0 holds them.
 * Replaces what Polars' rayon pool does for `.over(group)` (README.md:19) when more than one GPU is present. */
int pols_least_squares_sharded(pols_ctx *const *ctxs, pols_comm *const *comms, int n, const pols_batch *b, const pols_ols_params *p,
                               pols_out *o, int32_t out_mem);

#ifdef __cplusplus
}
#endif
#endif
